// thrl_tuple_stationary.hip -- greedy play under demand noise on the game's action tuples (thrl_tuple_stationary,
// include/thrl.h): the long-run distribution over the tuple played, by lazy power iteration of its Markov chain, for
// any mix of QTable, Reinforce and ActorCritic agents.  Two kernels.
//
// k_ts_chain: a 256-thread block per game, looping over games; both iterates m and the cell masses nu live in LDS.
//   Before the iteration the block groups the J cells by the tuple tau_g(k) they play and the T tuples by their
//   successor F_g(t): a bitonic sort of the 32-bit words (key << 16 | index), whose order IS the stable one since the
//   words are distinct, in scratch that aliases the second iterate and nu, which are dead until the first step.  What
//   stays is a permutation and the first place of every key (2 J + 6 T bytes), so D and Nn are segmented sums in
//   ascending index order by one thread per target tuple, and the reset distribution is one too.  nu is target-major
//   as in k_stationary: a thread carries two cells (k, k + 256) through the walk over the source tuples in ascending
//   order, m(t) and band_lo[t] are broadcasts, its band entries come from global memory (consecutive lanes, consecutive
//   addresses; the table is per config and stays in L2), and a wave leaves a tuple whose band misses all of its cells
//   after two compares.  The order of every add is the definition's whatever the scheduling; no atomic is involved.
//   The ordered output sums follow k_stationary: chunks of 64 tuples, one lane per tuple for the products, then one
//   lane per output reading them back in ascending t.
// k_ts_switch: one wavefront per game: the pairs of adjacent cells on which a network's entry differs, counted by
//   ballot, their widths added by lane 0 in ascending k.
#include "thrl_tuple_stationary.h"
#include "thrl_chain_dev.h"
#include "thrl_group_dev.h"

namespace thrl {

namespace {

__global__ void __launch_bounds__(kTsBlock) k_ts_chain(const TsArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N, G = a.G, T = a.T, J = a.J, W = a.W;
    double* ma = reinterpret_cast<double*>(s_mem + a.o_ma);
    double* mb = reinterpret_cast<double*>(s_mem + a.o_mb);
    double* nu = reinterpret_cast<double*>(s_mem + a.o_nu);
    double* prod = reinterpret_cast<double*>(s_mem + a.o_prod);       // [2N + 2][64]; its first words carry the wave maxima
    uint32_t* srt = reinterpret_cast<uint32_t*>(s_mem + a.o_mb);      // the groupings' scratch: over mb and nu
    uint16_t* permk = reinterpret_cast<uint16_t*>(s_mem + a.o_permk);
    uint16_t* firstk = reinterpret_cast<uint16_t*>(s_mem + a.o_startk);
    uint16_t* permt = reinterpret_cast<uint16_t*>(s_mem + a.o_permt);
    uint16_t* firstt = reinterpret_cast<uint16_t*>(s_mem + a.o_startt);
    const int n_out = 2 * N + 2;                                      // mass, N rewards, N actions, price

    for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
        const double p = a.noise_prob_g ? a.noise_prob_g[g] : a.noise_prob;
        const double q = __dsub_rn(1.0, p);
        bool ok = p > 0.0 && p <= 1.0;
        int t_start = -1;
        if (a.start_tuple) {
            t_start = a.start[g];
            ok = ok && t_start >= 0 && t_start < T;
        }
        if (!ok) {                                       // block-uniform: this game is not solved
            chain_unsolved(a.iters, a.change, a.mass, a.stat_price, a.stat_reward, a.stat_action, a.pi, g, G, N, T, tid, kTsBlock);
            continue;
        }

        // ---- the cells by the tuple they play, the tuples by their successor
        ts_group<kTsBlock>(a, a.cell_policy + g * N * J, nullptr, J, srt, permk, firstk, tid);
        ts_group<kTsBlock>(a, a.tuple_policy + g * N * T, nullptr, T, srt, permt, firstt, tid);

        for (int t = tid; t < T; t += kTsBlock) {
            double m0 = 0.0;
            if (a.start_tuple) {
                m0 = t == t_start ? 1.0 : 0.0;
            } else {
                const int e = firstk[t + 1];
                for (int s = firstk[t]; s < e; s++) m0 = __dadd_rn(m0, a.cell_w[permk[s]]);
            }
            ma[t] = m0;
        }
        __syncthreads();

        // ---- m' = m / 2 + s / 2 until the largest change is within tol
        double* mo = ma;
        double* mn = mb;
        int it = 0;
        double chg = 0.0;
        for (;;) {
            for (int k0 = tid; k0 < J; k0 += 2 * kTsBlock) {
                const int k1 = k0 + kTsBlock;
                const int kw = __builtin_amdgcn_readfirstlane(k0);    // the wave's cells: [kw, kw + 64) and 256 further
                double s0 = 0.0, s1 = 0.0;
                for (int t = 0; t < T; t++) {
                    const double m = mo[t];
                    if (m == 0.0) continue;              // the terms are +0.0: adding them changes nothing
                    const int blo = a.band_lo[t];
                    if (blo >= kw + kTsBlock + 64 || (int64_t)blo + W <= kw) continue;
                    const uint32_t d0 = (uint32_t)(k0 - blo), d1 = (uint32_t)(k1 - blo);
                    const double* __restrict__ row = a.band + (int64_t)t * W;
                    const double n0 = d0 < (uint32_t)W ? row[d0] : 0.0;
                    const double n1 = (d1 < (uint32_t)W && k1 < J) ? row[d1] : 0.0;
                    if (n0 != 0.0) s0 = __dadd_rn(s0, __dmul_rn(m, n0));
                    if (n1 != 0.0) s1 = __dadd_rn(s1, __dmul_rn(m, n1));
                }
                nu[k0] = s0;
                if (k1 < J) nu[k1] = s1;
            }
            __syncthreads();
            double c = 0.0;
            for (int t = tid; t < T; t += kTsBlock) {
                double d = 0.0, nn = 0.0;
                int e = firstt[t + 1];
                for (int s = firstt[t]; s < e; s++) d = __dadd_rn(d, mo[permt[s]]);
                e = firstk[t + 1];
                for (int s = firstk[t]; s < e; s++) nn = __dadd_rn(nn, nu[permk[s]]);
                const double sv = __dadd_rn(__dmul_rn(q, d), __dmul_rn(p, nn));
                mn[t] = chain_lazy(mo[t], sv, c);
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) c = fmax(c, __shfl_xor(c, m));
            if (lane == 0) prod[wave] = c;
            __syncthreads();
            c = fmax(fmax(prod[0], prod[1]), fmax(prod[2], prod[3]));
            double* tm = mo; mo = mn; mn = tm;
            it++;
            chg = c;
            if (c <= a.tol || it >= a.max_iters) break;
        }
        __syncthreads();                                 // the wave maxima are read before prod is staged over

        // ---- the outputs: chunks of 64 tuples, one lane per tuple, then one lane per ordered sum
        if (a.pi)
            for (int t = tid; t < T; t += kTsBlock) a.pi[g * T + t] = mo[t];
        double acc = 0.0;
        for (int t0 = 0; t0 < T; t0 += 64) {
            const int t = t0 + tid;
            if (tid < 64 && t < T) {
                const double m = mo[t];
                prod[tid] = m;
                for (int i = 0; i < N; i++) {
                    const double r = a.reward[(int64_t)i * T + t], nr = a.noise_reward[(int64_t)i * T + t];
                    prod[(1 + i) * 64 + tid] = __dmul_rn(m, __dadd_rn(__dmul_rn(q, r), __dmul_rn(p, nr)));
                    prod[(1 + N + i) * 64 + tid] = __dmul_rn(m, a.scaled[(int64_t)i * T + t]);
                }
                prod[(1 + 2 * N) * 64 + tid] = __dmul_rn(m, __dadd_rn(__dmul_rn(q, a.price[t]), __dmul_rn(p, a.noise_price[t])));
            }
            __syncthreads();
            const int n = min(64, T - t0);
            acc = chain_read_back(prod, n_out, n, acc, tid);
            __syncthreads();
        }
        chain_store(a.iters, a.change, a.mass, a.stat_price, a.stat_reward, a.stat_action, g, G, N, tid, it, chg, acc);
    }
}

__global__ void __launch_bounds__(256) k_ts_switch(const TsArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= a.G) return;
    const int J = a.J;
    const uint16_t* __restrict__ cp = a.cell_policy + g * a.N * J;
    int cnt = 0;
    double un = 0.0;
    for (int k0 = 0; k0 < J - 1; k0 += 64) {
        const int k = k0 + lane;
        bool f = false;
        if (k < J - 1)
            for (int i = 0; i < a.N; i++)
                if ((a.neural_mask >> i) & 1) {
                    const int top = a.n_actions[i] - 1;
                    f = f || min((int)cp[(int64_t)i * J + k], top) != min((int)cp[(int64_t)i * J + k + 1], top);
                }
        unsigned long long hit = __ballot(f);
        cnt += __popcll(hit);
        if (lane == 0)
            while (hit) {
                const int kk = k0 + __builtin_ctzll(hit);
                hit &= hit - 1;
                un = __dadd_rn(un, __dmul_rn(0.5, __dadd_rn(a.cell_w[kk], a.cell_w[kk + 1])));
            }
    }
    if (lane == 0) {
        if (a.n_switch) a.n_switch[g] = cnt;
        if (a.unresolved) a.unresolved[g] = un;
    }
}

}  // namespace

int launch_tuple_stationary(const TsArgs& a, int grid, hipStream_t s) {
    if (a.n_switch || a.unresolved) {
        hipLaunchKernelGGL(k_ts_switch, dim3((unsigned)((a.G + 3) / 4)), dim3(256), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    if (a.lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_ts_chain),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, a.lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k_ts_chain, dim3(grid), dim3(kTsBlock), (size_t)a.lds_bytes, s, a);
    return (int)hipGetLastError();
}

}  // namespace thrl
