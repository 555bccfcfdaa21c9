// thrl_tuple_deviation_noise.hip -- the deviation test under demand noise on the game's action tuples
// (thrl_tuple_deviation_noise, include/thrl.h): the expected impulse response of noisy greedy play to a forced deviation,
// for any mix of QTable, Reinforce and ActorCritic agents, by propagating a distribution over the tuple greedy play
// intends through the chain of thrl_tuple_stationary -- L plain steps with the deviator's action replaced in the tuple
// played, then K - L plain steps of the greedy chain -- and what every period's distribution earns.
//
// k_tdn_chain has k_ts_chain's shape: a 256-thread block per game, looping over games; both iterates and the cell masses
// nu live in LDS.  Once per game the block computes Dv_g (the tuple played in place of t while the deviation lasts,
// uint16 [T]: T * A_d evaluations of R_d for a best response) and three stable groupings by ts_group: the cells by the
// tuple tau_g(k) they play, the tuples by F_g(Dv_g(t)) and the tuples by F_g(t), in scratch that aliases the second
// iterate and nu, which are dead until the first step.  A step is k_ts_chain's without the lazy half: nu target-major, a
// thread carrying two cells (k, k + 256) through the walk over the source tuples in ascending order, m(t) and the tuple
// played e(t) as LDS broadcasts, band_lo and the thread's band entries of e(t)'s row from global memory, a wave leaving
// a source whose band misses all of its cells; then D and Nn as segmented sums in ascending index order by one thread
// per target tuple.  The ordered sums of a period follow k_ts_chain's outputs: chunks of 64 tuples, one lane per tuple
// for the products, then one lane per sum reading them back in ascending t.  The lane of a sum keeps what is derived
// from it in registers over the periods, as k_deviation_noise does: lane d the gain and the low, lane 2N the distance
// and ret_step.  m_0 is re-read from global memory (coalesced) for the distance.  No atomic is involved.
#include "thrl_tuple_deviation_noise.h"
#include "thrl_solve_dev.h"
#include "thrl_group_dev.h"

namespace thrl {

namespace {

__global__ void __launch_bounds__(kTdnBlock) k_tdn_chain(const TdnArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    const int tid = threadIdx.x;
    const int N = a.N, G = a.G, T = a.T, J = a.J, W = a.W, K = a.K, L = a.L, d = a.d;
    double* ma = reinterpret_cast<double*>(s_mem + a.o_ma);
    double* mb = reinterpret_cast<double*>(s_mem + a.o_mb);
    double* nu = reinterpret_cast<double*>(s_mem + a.o_nu);
    double* prod = reinterpret_cast<double*>(s_mem + a.o_prod);       // [2N + 2][64] the chunk's terms per sum
    uint32_t* srt = reinterpret_cast<uint32_t*>(s_mem + a.o_mb);      // the groupings' scratch: over mb and nu
    uint16_t* permk = reinterpret_cast<uint16_t*>(s_mem + a.o_permk);
    uint16_t* firstk = reinterpret_cast<uint16_t*>(s_mem + a.o_startk);
    uint16_t* permd = reinterpret_cast<uint16_t*>(s_mem + a.o_permd);
    uint16_t* firstd = reinterpret_cast<uint16_t*>(s_mem + a.o_startd);
    uint16_t* permt = reinterpret_cast<uint16_t*>(s_mem + a.o_permt);
    uint16_t* firstt = reinterpret_cast<uint16_t*>(s_mem + a.o_startt);
    uint16_t* dv = reinterpret_cast<uint16_t*>(s_mem + a.o_dv);       // Dv_g(t)
    const int n_out = 2 * N + 2;                                      // N rewards, N actions, distance / share, mass
    const int rb = a.row_begin, rc = a.row_count;

    for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
        const double* __restrict__ w0 = a.weights + g * T;
        const double p = a.noise_prob_g ? a.noise_prob_g[g] : a.noise_prob;
        const double q = __dsub_rn(1.0, p);
        if (!(p > 0.0 && p <= 1.0)) {                    // block-uniform: this game is not solved
            if (tid < N) {
                a.base_reward[(int64_t)tid * G + g] = 0.0;
                a.base_action[(int64_t)tid * G + g] = 0.0;
            }
            if (tid == 0) {
                a.dev_share[g] = 0.0; a.gain[g] = 0.0; a.gain_dev[g] = 0.0; a.low[g] = 0.0; a.dist[g] = 0.0; a.mass[g] = 0.0;
                a.low_step[g] = -1; a.ret_step[g] = -1;
            }
            for (int r = tid; r < rc * N; r += kTdnBlock) {
                if (a.reward_rows) a.reward_rows[(int64_t)r * G + g] = 0.0;
                if (a.action_rows) a.action_rows[(int64_t)r * G + g] = 0.0;
            }
            if (a.dist_rows)
                for (int r = tid; r < rc; r += kTdnBlock) a.dist_rows[(int64_t)r * G + g] = 0.0;
            continue;
        }

        // ---- Dv_g, then the cells by the tuple they play, the tuples by F_g o Dv_g and by F_g, and m_0
        {
            const int ts = a.tstride[d], nd = a.n_actions[d];
            const double* __restrict__ rd = a.reward + (int64_t)d * T;
            const double* __restrict__ nr = a.noise_reward + (int64_t)d * T;
            for (int t = tid; t < T; t += kTdnBlock) {
                const int cur = (t / ts) % nd;
                int ad = a.dev_action;
                if (ad < 0) {                            // d's one-period best response to the rivals' actions in t
                    const int t0 = t - cur * ts;
                    double best;
                    ad = first_max(nd, [&](int b) THRL_SOLVE_INLINE {
                        return noise_blend(q, rd[t0 + b * ts], p, nr[t0 + b * ts]);
                    }, best);
                }
                dv[t] = (uint16_t)(t + (ad - cur) * ts);
            }
        }
        ts_group<kTdnBlock>(a, a.cell_policy + g * N * J, nullptr, J, srt, permk, firstk, tid);
        ts_group<kTdnBlock>(a, a.tuple_policy + g * N * T, dv, T, srt, permd, firstd, tid);
        ts_group<kTdnBlock>(a, a.tuple_policy + g * N * T, nullptr, T, srt, permt, firstt, tid);
        for (int t = tid; t < T; t += kTdnBlock) ma[t] = w0[t];
        __syncthreads();

        // the ordered sums of one distribution m, the tuple played in place of t being dv[t] (dev) or t; thread o < n_out
        // its own: o < N the reward of agent o, N <= o < 2N the action of agent o - N, 2N the sum of |m - m_0| (base: of
        // m where Dv(t) != t), 2N + 1 m
        auto sums = [&](const double* m, bool dev, bool base) -> double {
            double acc = 0.0;
            for (int t0 = 0; t0 < T; t0 += 64) {
                const int t = t0 + tid;
                if (tid < 64 && t < T) {
                    const int te = dev ? (int)dv[t] : t;
                    const double mt = m[t];
                    for (int i = 0; i < N; i++) {
                        const double r = a.reward[(int64_t)i * T + te], nr = a.noise_reward[(int64_t)i * T + te];
                        prod[i * 64 + tid] = __dmul_rn(mt, noise_blend(q, r, p, nr));
                        prod[(N + i) * 64 + tid] = __dmul_rn(mt, a.scaled[(int64_t)i * T + te]);
                    }
                    prod[2 * N * 64 + tid] = base ? ((int)dv[t] != t ? mt : 0.0) : fabs(__dsub_rn(mt, w0[t]));
                    prod[(2 * N + 1) * 64 + tid] = mt;
                }
                __syncthreads();
                acc = chain_read_back(prod, n_out, min(64, T - t0), acc, tid);
                __syncthreads();
            }
            return acc;
        };

        // ---- the baseline: what m_0 earns under greedy play, and the share of it the deviation changes
        double acc = sums(ma, false, true);
        const double base = acc;                         // thread i < N: base_reward_i
        if (tid < N) a.base_reward[(int64_t)tid * G + g] = acc;
        else if (tid < 2 * N) a.base_action[(int64_t)(tid - N) * G + g] = acc;
        else if (tid == 2 * N) a.dev_share[g] = acc;

        // ---- K periods: the sums of m_tau, then the plain step m_{tau+1}; D(K) and the mass after them
        const double gam = a.sweep_gamma ? a.sweep_gamma[(int64_t)d * G + g] : a.gamma_d;
        double w = 1.0, gain = 0.0, gain_dev = 0.0, low = 0.0, D = 0.0;
        int low_step = -1, ret = -1;
        double* mo = ma;
        double* mn = mb;
        for (int tau = 0;; tau++) {
            const bool dev = tau < L;
            acc = sums(mo, dev, false);
            D = __dmul_rn(0.5, acc);                     // the distance, on thread 2N
            if (tau < K) {
                if (tid == d) {
                    const double diff = __dsub_rn(acc, base);
                    const double term = __dmul_rn(w, diff);
                    gain = __dadd_rn(gain, term);
                    if (tau < L) {
                        gain_dev = __dadd_rn(gain_dev, term);
                    } else if (tau == L || diff < low) {
                        low = diff;
                        low_step = tau;
                    }
                    w = __dmul_rn(w, gam);
                }
                const int r = tau - rb;
                if (r >= 0 && r < rc) {
                    if (tid < N) {
                        if (a.reward_rows) a.reward_rows[((int64_t)r * N + tid) * G + g] = acc;
                    } else if (tid < 2 * N) {
                        if (a.action_rows) a.action_rows[((int64_t)r * N + (tid - N)) * G + g] = acc;
                    } else if (tid == 2 * N) {
                        if (a.dist_rows) a.dist_rows[(int64_t)r * G + g] = D;
                    }
                }
            }
            if (tid == 2 * N && tau >= L && ret < 0 && D <= a.ret_tol) ret = tau;
            if (tau == K) break;

            // nu(k) = sum_t m(t) n(e(t), k), target-major
            for (int k0 = tid; k0 < J; k0 += 2 * kTdnBlock) {
                const int k1 = k0 + kTdnBlock;
                const int kw = __builtin_amdgcn_readfirstlane(k0);    // the wave's cells: [kw, kw + 64) and 256 further
                double s0 = 0.0, s1 = 0.0;
                for (int t = 0; t < T; t++) {
                    const double m = mo[t];
                    if (m == 0.0) continue;              // the terms are +0.0: adding them changes nothing
                    const int te = dev ? (int)dv[t] : t;
                    const int blo = a.band_lo[te];
                    if (blo >= kw + kTdnBlock + 64 || (int64_t)blo + W <= kw) continue;
                    const uint32_t d0 = (uint32_t)(k0 - blo), d1 = (uint32_t)(k1 - blo);
                    const double* __restrict__ row = a.band + (int64_t)te * W;
                    const double n0 = d0 < (uint32_t)W ? row[d0] : 0.0;
                    const double n1 = (d1 < (uint32_t)W && k1 < J) ? row[d1] : 0.0;
                    if (n0 != 0.0) s0 = __dadd_rn(s0, __dmul_rn(m, n0));
                    if (n1 != 0.0) s1 = __dadd_rn(s1, __dmul_rn(m, n1));
                }
                nu[k0] = s0;
                if (k1 < J) nu[k1] = s1;
            }
            __syncthreads();
            // m'(t') = q D(t') + p Nn(t')
            const uint16_t* perm = dev ? permd : permt;
            const uint16_t* first = dev ? firstd : firstt;
            for (int t = tid; t < T; t += kTdnBlock) {
                double dd = 0.0, nn = 0.0;
                int e = first[t + 1];
                for (int s = first[t]; s < e; s++) dd = __dadd_rn(dd, mo[perm[s]]);
                e = firstk[t + 1];
                for (int s = firstk[t]; s < e; s++) nn = __dadd_rn(nn, nu[permk[s]]);
                mn[t] = __dadd_rn(__dmul_rn(q, dd), __dmul_rn(p, nn));
            }
            __syncthreads();
            double* tm = mo; mo = mn; mn = tm;
        }
        if (tid == d) {
            a.gain[g] = gain; a.gain_dev[g] = gain_dev; a.low[g] = low; a.low_step[g] = low_step;
        }
        if (tid == 2 * N) {
            a.ret_step[g] = ret; a.dist[g] = D;
        } else if (tid == 2 * N + 1) {
            a.mass[g] = acc;
        }
        __syncthreads();                                 // this game's LDS reads before the next game's writes
    }
}

}  // namespace

int launch_tuple_deviation_noise(const TdnArgs& a, int grid, hipStream_t s) {
    if (a.lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_tdn_chain),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, a.lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k_tdn_chain, dim3(grid), dim3(kTdnBlock), (size_t)a.lds_bytes, s, a);
    return (int)hipGetLastError();
}

}  // namespace thrl
