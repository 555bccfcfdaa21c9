// thrl_sampled.hip -- sampled play on the game's action tuples (thrl_sampled_chain, include/thrl.h): the long-run
// distribution over the tuple played when every agent SAMPLES its action (a network from its softmax, a QTable agent
// epsilon-greedily), by lazy power iteration of the chain P(t -> t') = prod_i pi_i(a_i(t') | price(t)).  One kernel.
//
// k_sp_chain: a 256-thread block per game, looping over games.  The transition row depends on t only through its price,
//   so the block keeps per DISTINCT price d: the mass M(d) on the tuples with that price, divided by the normaliser
//   Z(d) into W(d); the float32 probability rows of the networks, row-major [d][k]; and for a QTable agent its greedy
//   action at d (2 bytes) beside two per-game constants.  The grouping of the tuples by price is per config: it is staged
//   once per block, clamped, so M(d) is a segmented sum in ascending t by one thread per d.  A thread owns output tuples
//   t' and walks d ascending: W(d) is a broadcast (and the skip of an empty d is block-uniform), the rows of the last
//   agent are read at consecutive words by consecutive lanes, those of the slower agents by runs of lanes at one word.
//   The ordered sum over d forbids a split over d and any matrix instruction; the parallelism is across t'.  The largest
//   change is a maximum, whose order is free: it goes through LDS in two levels, no shuffle.  The ordered output sums
//   follow k_ts_chain: chunks of 64 tuples, one lane per tuple for the products, then one lane per output reading them
//   back in ascending t; `agree` is one more lane over the D terms parked in the dead iterate.
//   The body is calls: the staging, Z(d), the M / W pass, the sum over the distinct prices, the block maximum and agree's
//   terms are thrl_sampled_dev.h's, shared with k_spn_chain; the unsolved outputs, the lazy update, the read-back and the
//   final store are thrl_chain_dev.h's, shared with all four chain kernels.  Only the staging of the products is here.
//   Nothing in the body is wave-specific: with THRL_SP_HOST_BUILD the same source runs as 256 host threads with barriers.
#include "thrl_sampled_dev.h"

namespace thrl {

namespace {

template <int MAXN>
__device__ __forceinline__ void sp_block(const SpArgs& a, unsigned char* s_mem, int tid, int bid, int nblk) {
    const int N = a.N, G = a.G, T = a.T, D = a.D;
    double* ma = reinterpret_cast<double*>(s_mem + a.o_ma);
    double* mb = reinterpret_cast<double*>(s_mem + a.o_mb);
    double* W = reinterpret_cast<double*>(s_mem + a.o_w);
    double* Z = reinterpret_cast<double*>(s_mem + a.o_z);
    uint16_t* first = reinterpret_cast<uint16_t*>(s_mem + a.o_first);
    uint16_t* perm = reinterpret_cast<uint16_t*>(s_mem + a.o_perm);
    double* prod = reinterpret_cast<double*>(s_mem + a.o_prod);       // [2N + 2][64] >= 256 words: also the threads' maxima
    SpCst* cst = reinterpret_cast<SpCst*>(s_mem + a.o_cst);
    const int n_out = 2 * N + 2;                                      // mass, N rewards, N actions, price

    // ---- the grouping of the tuples by price: per config, staged once; no entry leads out of bounds
    for (int d = tid; d <= D; d += kSpBlock) first[d] = (uint16_t)min(max(a.grp_first[d], 0), T);
    for (int t = tid; t < T; t += kSpBlock) perm[t] = (uint16_t)min(max(a.grp_perm[t], 0), T - 1);

    for (int64_t g = bid; g < G; g += nblk) {
        bool ok = sp_eps_ok(a, g);
        int t_start = -1;
        if (a.start_tuple) {
            t_start = a.start[g];
            ok = ok && t_start >= 0 && t_start < T;
        }
        if (!ok) {                                       // block-uniform: this game is not solved
            chain_unsolved(a.iters, a.change, a.mass, a.samp_price, a.samp_reward, a.samp_action, a.pi, g, G, N, T, tid, kSpBlock);
            if (tid == 0) a.agree[g] = 0.0;
            continue;
        }
        __syncthreads();                                 // the game before is read to its end; the grouping is staged

        // ---- the game's rows and constants
        sp_stage_game<1>(a, s_mem, cst, g, tid);
        __syncthreads();
        sp_normaliser(a, s_mem, Z, tid);
        const double unif = __ddiv_rn(1.0, (double)T);
        for (int t = tid; t < T; t += kSpBlock) ma[t] = a.start_tuple ? (t == t_start ? 1.0 : 0.0) : unif;
        __syncthreads();

        // ---- m' = m / 2 + s / 2 until the largest change is within tol
        double* mo = ma;
        double* mn = mb;
        int it = 0;
        double chg = 0.0;
        for (;;) {
            sp_weights(a, mo, first, perm, Z, W, tid);
            __syncthreads();
            double c = 0.0;
            for (int t = tid; t < T; t += kSpBlock) {
                int off[MAXN];
                sp_offsets<MAXN>(a, t, off);
                const double s = sp_price_sum<MAXN>(a, s_mem, cst, W, off);
                mn[t] = chain_lazy(mo[t], s, c);
            }
            c = sp_block_max(prod, cst, c, tid);
            double* tm = mo; mo = mn; mn = tm;
            it++;
            chg = c;
            if (c <= a.tol || it >= a.max_iters) break;
        }
        __syncthreads();                                 // the maxima are read before prod is staged over

        // ---- the outputs, from the last iterate
        sp_weights(a, mo, first, perm, Z, W, tid);
        __syncthreads();
        sp_agree_terms(a, s_mem, cst, W, mn, g, tid);    // parked in the dead iterate (D <= T)
        if (a.pi)
            for (int t = tid; t < T; t += kSpBlock) a.pi[g * T + t] = mo[t];
        double acc = 0.0;
        for (int t0 = 0; t0 < T; t0 += 64) {
            const int t = t0 + tid;
            if (tid < 64 && t < T) {
                const double m = mo[t];
                prod[tid] = m;
                for (int i = 0; i < N; i++) {
                    prod[(1 + i) * 64 + tid] = __dmul_rn(m, a.reward[(int64_t)i * T + t]);
                    prod[(1 + N + i) * 64 + tid] = __dmul_rn(m, a.scaled[(int64_t)i * T + t]);
                }
                prod[(1 + 2 * N) * 64 + tid] = __dmul_rn(m, a.price[t]);
            }
            __syncthreads();
            acc = chain_read_back(prod, n_out, min(64, T - t0), acc, tid);
            if (tid == 64 && t0 == 0)
                for (int d = 0; d < D; d++) acc = __dadd_rn(acc, mn[d]);
            __syncthreads();
        }
        chain_store(a.iters, a.change, a.mass, a.samp_price, a.samp_reward, a.samp_action, g, G, N, tid, it, chg, acc);
        if (tid == 64) a.agree[g] = acc;
    }
}

#ifndef THRL_SP_HOST_BUILD
template <int MAXN>
__global__ void __launch_bounds__(kSpBlock) k_sp_chain(const SpArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    sp_block<MAXN>(a, s_mem, (int)threadIdx.x, (int)blockIdx.x, (int)gridDim.x);
}
#endif

}  // namespace

#ifndef THRL_SP_HOST_BUILD
int launch_sampled_chain(const SpArgs& a, int grid, hipStream_t s) {
    return sp_launch(k_sp_chain<2>, k_sp_chain<kSpMaxA>, a, a, grid, s);
}
#endif

}  // namespace thrl
