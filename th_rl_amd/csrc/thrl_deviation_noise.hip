// thrl_deviation_noise.hip -- the deviation test under demand noise (thrl_deviation_noise, include/thrl.h): the expected
// impulse response of a game's noisy greedy play to a forced deviation, by propagating a distribution over the price
// cells through the chain of thrl_stationary -- L plain steps of the chain with the deviator's action replaced in
// every cell, then K - L steps of the greedy chain -- and what every period's distribution earns.
//
// One wavefront (a one-wave block) per game, looping over games, as k_stationary.  LDS holds the two iterates, the
// tuples t(k) and t'(k) of every cell and the [2N + 2][64] staging of the ordered sums; m_0 is re-read from global
// memory (coalesced) once per period for the distance D(tau).  The step is k_stationary's target-major walk in its
// form without per-cell tables, always: every lane walks the sources j in ascending order, reads m(j) and the source's
// tuple as LDS broadcasts, the tuple's det_cell / band_lo entries (wave-uniform addresses) and its own band entry from
// global memory (consecutive lanes, consecutive addresses; the tables are shared by all games and stay in L2), so the
// order of the adds is the definition's and no atomic is involved.  A lane carries two targets (k, k + 64) through one
// walk.  The ordered sums of a period follow k_stationary's outputs: chunks of 64 cells, one lane per cell for the
// products, then one lane per sum reading them back from LDS in ascending k.  The lane of a sum keeps what is derived
// from it in registers over the periods: lane d the gain, lane 2N the distance and ret_step.
#include "thrl_deviation_noise.h"
#include "thrl_solve_dev.h"

namespace thrl {

namespace {

__global__ void __launch_bounds__(64) k_deviation_noise(const DevnArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    const int lane = threadIdx.x;
    const int N = a.N, G = a.G, J = a.J, W = a.W, TT = a.T, K = a.K, L = a.L, d = a.d;
    double* mua = reinterpret_cast<double*>(s_mem + a.o_mua);
    double* mub = reinterpret_cast<double*>(s_mem + a.o_mub);
    double* prod = reinterpret_cast<double*>(s_mem + a.o_prod);       // [2N + 2][64] the chunk's terms per sum
    uint16_t* tup = reinterpret_cast<uint16_t*>(s_mem + a.o_tup);     // t(k)
    uint16_t* tupd = reinterpret_cast<uint16_t*>(s_mem + a.o_tupd);   // t'(k)
    const int n_out = 2 * N + 2;                                      // N rewards, N actions, distance / share, mass
    const int rb = a.row_begin, rc = a.row_count;

    for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
        const uint16_t* __restrict__ pg = a.policy + g * a.P;
        const double* __restrict__ w0 = a.weights + g * J;
        const double p = a.noise_prob_g ? a.noise_prob_g[g] : a.noise_prob;
        const double q = __dsub_rn(1.0, p);
        if (!(p > 0.0 && p <= 1.0)) {                    // wave-uniform: this game is not solved
            if (lane < N) {
                a.base_reward[(int64_t)lane * G + g] = 0.0;
                a.base_action[(int64_t)lane * G + g] = 0.0;
            }
            if (lane == 0) {
                a.dev_share[g] = 0.0; a.gain[g] = 0.0; a.gain_dev[g] = 0.0; a.low[g] = 0.0; a.dist[g] = 0.0; a.mass[g] = 0.0;
                a.low_step[g] = -1; a.ret_step[g] = -1;
            }
            for (int r = lane; r < rc * N; r += 64) {
                if (a.reward_rows) a.reward_rows[(int64_t)r * G + g] = 0.0;
                if (a.action_rows) a.action_rows[(int64_t)r * G + g] = 0.0;
            }
            if (a.dist_rows)
                for (int r = lane; r < rc; r += 64) a.dist_rows[(int64_t)r * G + g] = 0.0;
            __syncthreads();
            continue;
        }

        // ---- the tuples t(k) and t'(k) of every cell, and m_0
        for (int k = lane; k < J; k += 64) {
            int t = 0, cur = 0;
            for (int i = 0; i < N; i++) {
                const int row = clamp_row(a.cell_rows[(int64_t)i * J + k], a.ag[i]);
                const int ai = row_action(a, pg, i, row);
                t += ai * a.tstride[i];
                if (i == d) cur = ai;
            }
            int ad = a.dev_action;
            if (ad < 0) {                                // d's one-period best response in this cell
                const int ts = a.tstride[d];
                const int t0 = t - cur * ts;
                const double* __restrict__ rd = a.rew + (int64_t)d * TT;
                const double* __restrict__ nd = a.noise_reward + (int64_t)d * TT;
                double best;
                ad = first_max(a.ag[d].n_actions, [&](int b) THRL_SOLVE_INLINE {
                    return noise_blend(q, rd[t0 + b * ts], p, nd[t0 + b * ts]);
                }, best);
            }
            tup[k] = (uint16_t)t;
            tupd[k] = (uint16_t)(t + (ad - cur) * a.tstride[d]);
            mua[k] = w0[k];
        }
        __syncthreads();

        // the ordered sums of one distribution m under the tuples tc, lane o < n_out its own: o < N the reward of
        // agent o, N <= o < 2N the action of agent o - N, 2N the sum of |m - m_0| (base: of m where t' != t), 2N + 1 m
        auto sums = [&](const double* m, const uint16_t* tc, bool base) -> double {
            double acc = 0.0;
            for (int k0 = 0; k0 < J; k0 += 64) {
                const int k = k0 + lane;
                if (k < J) {
                    const int t = tc[k];
                    const double mk = m[k];
                    int rest = t;
                    for (int i = 0; i < N; i++) {
                        const int ai = rest / a.tstride[i];
                        rest -= ai * a.tstride[i];
                        const double r = a.rew[(int64_t)i * TT + t], nr = a.noise_reward[(int64_t)i * TT + t];
                        prod[i * 64 + lane] = __dmul_rn(mk, noise_blend(q, r, p, nr));
                        prod[(N + i) * 64 + lane] = __dmul_rn(mk, scale_action(ai, a.ag[i]));
                    }
                    prod[2 * N * 64 + lane] = base ? ((int)tupd[k] != t ? mk : 0.0) : fabs(__dsub_rn(mk, w0[k]));
                    prod[(2 * N + 1) * 64 + lane] = mk;
                }
                __syncthreads();
                acc = chain_read_back(prod, n_out, min(64, J - k0), acc, lane);
                __syncthreads();
            }
            return acc;
        };

        // ---- the baseline: what m_0 earns under greedy play, and the share of it the deviation changes
        double acc = sums(mua, tup, true);
        const double base = acc;                         // lane i < N: base_reward_i
        if (lane < N) a.base_reward[(int64_t)lane * G + g] = acc;
        else if (lane < 2 * N) a.base_action[(int64_t)(lane - N) * G + g] = acc;
        else if (lane == 2 * N) a.dev_share[g] = acc;

        // ---- K periods: the sums of m_tau, then the plain step m_{tau+1} = m_tau P^(tau); D(K) and the mass after them
        const double gam = a.sweep_gamma ? a.sweep_gamma[(int64_t)d * G + g] : a.gamma_d;
        double w = 1.0, gain = 0.0, gain_dev = 0.0, low = 0.0, D = 0.0;
        int low_step = -1, ret = -1;
        double* mo = mua;
        double* mn = mub;
        for (int tau = 0;; tau++) {
            const uint16_t* tc = tau < L ? tupd : tup;
            acc = sums(mo, tc, false);
            D = __dmul_rn(0.5, acc);                     // the distance, on lane 2N
            if (tau < K) {
                if (lane == d) {
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
                    if (lane < N) {
                        if (a.reward_rows) a.reward_rows[((int64_t)r * N + lane) * G + g] = acc;
                    } else if (lane < 2 * N) {
                        if (a.action_rows) a.action_rows[((int64_t)r * N + (lane - N)) * G + g] = acc;
                    } else if (lane == 2 * N) {
                        if (a.dist_rows) a.dist_rows[(int64_t)r * G + g] = D;
                    }
                }
            }
            if (lane == 2 * N && tau >= L && ret < 0 && D <= a.ret_tol) ret = tau;
            if (tau == K) break;

            for (int k0 = lane; k0 < J; k0 += 128) {
                const int k1 = k0 + 64;
                double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
                for (int j = 0; j < J; j++) {
                    const double m = mo[j];
                    if (m == 0.0) continue;              // the terms are +0.0: adding them changes nothing
                    const int t = tc[j];
                    const int blo = a.band_lo[t];
                    const int dc = a.det_cell[t];
                    const int det = (dc >= 0 && dc < J) ? dc : 0xffff;
                    const uint32_t boff = (uint32_t)(t * W) - (uint32_t)blo;
                    const uint32_t d0 = (uint32_t)(k0 - blo), d1 = (uint32_t)(k1 - blo);
                    const double n0 = d0 < (uint32_t)W ? a.band[boff + (uint32_t)k0] : 0.0;
                    const double n1 = (d1 < (uint32_t)W && k1 < J) ? a.band[boff + (uint32_t)k1] : 0.0;
                    const double pn0 = __dmul_rn(p, n0), pn1 = __dmul_rn(p, n1);
                    const double P0 = det == k0 ? __dadd_rn(q, pn0) : pn0;
                    const double P1 = det == k1 ? __dadd_rn(q, pn1) : pn1;
                    if (P0 != 0.0) s0 = __dadd_rn(s0, __dmul_rn(m, P0));
                    if (P1 != 0.0) s1 = __dadd_rn(s1, __dmul_rn(m, P1));
                }
                mn[k0] = s0;
                if (k1 < J) mn[k1] = s1;
            }
            __syncthreads();
            double* tm = mo; mo = mn; mn = tm;
        }
        if (lane == d) {
            a.gain[g] = gain; a.gain_dev[g] = gain_dev; a.low[g] = low; a.low_step[g] = low_step;
        }
        if (lane == 2 * N) {
            a.ret_step[g] = ret; a.dist[g] = D;
        } else if (lane == 2 * N + 1) {
            a.mass[g] = acc;
        }
        __syncthreads();                                 // this game's LDS reads before the next game's writes
    }
}

}  // namespace

int launch_deviation_noise(const DevnArgs& a, int grid, hipStream_t s) {
    hipLaunchKernelGGL(k_deviation_noise, dim3(grid), dim3(64), (size_t)a.lds_bytes, s, a);
    return (int)hipGetLastError();
}

}  // namespace thrl
