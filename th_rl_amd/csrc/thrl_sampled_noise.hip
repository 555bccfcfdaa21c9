// thrl_sampled_noise.hip -- sampled play under demand noise (thrl_sampled_noise_chain, include/thrl.h): k_sp_chain's
// chain with the environment's redraw of the demand intercept.  With probability q = 1 - p the next price is the tuple's
// noise-free price (k_sp_chain's half, over the D distinct prices); with probability p it is uniform on the tuple's band
// of the price axis, and the networks' probabilities at a redrawn price are taken at the quadrature nodes xn (k_ts_chain's
// half, with probability rows where that kernel has one greedy action).  Two kernels.
//
// k_spn_chain: a 256-thread block per game, looping over games, a thread owns output tuples t'.  The M / W pass, the
//   ordered sum over the distinct prices and the block maximum are thrl_sampled_dev.h's, shared with k_sp_chain.  nu is
//   gathered target-major as in k_ts_chain: a thread carries its nodes through the ascending walk over t, m(t) and
//   band_lo[t] are broadcasts, a wave leaves a tuple whose band misses its nodes.  The node rows of the networks
//   (4 Jn A_i bytes each) do not fit beside the distinct-price rows, and they are not needed at once: they are streamed
//   from global memory in ascending j through two LDS buffers of kSpnTile nodes per network, register-staged: the 16-byte
//   loads of tile k + 1 are issued before the arithmetic on tile k and written to the other buffer after it (one
//   barrier).  A tile starts wherever (g Jn + j0) A_i floats fall, so the words are taken from the 16-byte boundary below
//   it and the buffer keeps that lead; the two ragged words are loaded float by float, nothing outside the rows is read.
//   Zn(j) is recomputed from the tile's rows by one lane per node each time the tile is resident (V(j) = nu(j) / Zn(j) in
//   place: one more barrier); it is not kept.  Partial sums of Sn(t') between tiles live in the iterate being written,
//   which only the owning thread touches, so the order over j is the plain ascending one.  The reset start is the same
//   pass with node_w as numerator; agree's noise half is the pass without the accumulation, its terms parked in V.
//   The node half (the tiles, nu and the walk over the nodes) sits in thrl_sampled_noise_dev.h, shared with k_sdn_chain
//   (thrl_sampled_deviation_noise.hip).
// k_spn_jump: max_jump, the largest change of a network's probability between adjacent nodes, for every game.
//   Nothing in the bodies is wave-specific: with THRL_SP_HOST_BUILD the same source runs as 256 host threads with barriers.
#include "thrl_sampled_noise.h"
#include "thrl_sampled_noise_dev.h"

namespace thrl {

namespace {

template <int MAXN>
__device__ __forceinline__ void spn_block(const SpnArgs& a, unsigned char* s_mem, int tid, int bid, int nblk) {
    const SpArgs& sa = a.sp;
    const int N = sa.N, G = sa.G, T = sa.T, D = sa.D, Jn = a.Jn;
    double* ma = reinterpret_cast<double*>(s_mem + sa.o_ma);
    double* mb = reinterpret_cast<double*>(s_mem + sa.o_mb);
    double* W = reinterpret_cast<double*>(s_mem + sa.o_w);
    double* Z = reinterpret_cast<double*>(s_mem + sa.o_z);
    double* V = reinterpret_cast<double*>(s_mem + a.o_v);
    uint16_t* first = reinterpret_cast<uint16_t*>(s_mem + sa.o_first);
    uint16_t* perm = reinterpret_cast<uint16_t*>(s_mem + sa.o_perm);
    double* prod = reinterpret_cast<double*>(s_mem + sa.o_prod);      // [2N + 2][64] >= 256 words: also the threads' maxima
    SpCst* cst = reinterpret_cast<SpCst*>(s_mem + sa.o_cst);
    const int n_out = 2 * N + 2;                                      // mass, N rewards, N actions, price

    // ---- the grouping of the tuples by price: per config, staged once; no entry leads out of bounds
    for (int d = tid; d <= D; d += kSpBlock) first[d] = (uint16_t)min(max(sa.grp_first[d], 0), T);
    for (int t = tid; t < T; t += kSpBlock) perm[t] = (uint16_t)min(max(sa.grp_perm[t], 0), T - 1);

    for (int64_t g = bid; g < G; g += nblk) {
        const double p = a.noise_prob_g ? a.noise_prob_g[g] : a.noise_prob;
        const double q = __dsub_rn(1.0, p);
        bool ok = sp_eps_ok(sa, g) && p >= 0.0 && p <= 1.0;
        int t_start = -1;
        if (sa.start_tuple) {
            t_start = sa.start[g];
            ok = ok && t_start >= 0 && t_start < T;
        }
        if (!ok) {                                       // block-uniform: this game is not solved
            chain_unsolved(sa.iters, sa.change, sa.mass, sa.samp_price, sa.samp_reward, sa.samp_action, sa.pi, g, G, N, T, tid, kSpBlock);
            if (tid == 0) sa.agree[g] = 0.0;
            continue;
        }
        __syncthreads();                                 // the game before is read to its end; the grouping is staged

        // ---- the game's rows and constants; the QTable agents' entries at the nodes
        sp_stage_game<2>(sa, s_mem, cst, g, tid);
        for (int i = 0; i < N; i++)
            if (sa.kind[i] == 0) {
                uint16_t* nq = reinterpret_cast<uint16_t*>(s_mem + a.o_nrow[i]);
                const uint16_t* __restrict__ src = a.npolicy + (g * N + i) * Jn;
                for (int j = tid; j < Jn; j += kSpBlock) nq[j] = (uint16_t)min((int)src[j], sa.n_actions[i] - 1);
            }
        if (a.start_reset)
            for (int j = tid; j < Jn; j += kSpBlock) V[j] = a.node_w[j];
        __syncthreads();
        sp_normaliser(sa, s_mem, Z, tid);
        if (a.start_reset) {
            spn_node_pass<MAXN, true>(a, s_mem, cst, V, ma, true, g, tid);
        } else {
            const double unif = __ddiv_rn(1.0, (double)T);
            for (int t = tid; t < T; t += kSpBlock) ma[t] = sa.start_tuple ? (t == t_start ? 1.0 : 0.0) : unif;
        }
        __syncthreads();

        // ---- m' = m / 2 + s / 2 until the largest change is within tol
        double* mo = ma;
        double* mn = mb;
        int it = 0;
        double chg = 0.0;
        for (;;) {
            sp_weights(sa, mo, first, perm, Z, W, tid);
            spn_nu(a, mo, V, tid);
            __syncthreads();
            spn_node_pass<MAXN, true>(a, s_mem, cst, V, mn, false, g, tid);     // Sn(t') into the iterate being written
            double c = 0.0;
            for (int t = tid; t < T; t += kSpBlock) {
                int off[MAXN];
                sp_offsets<MAXN>(sa, t, off);
                const double sd = sp_price_sum<MAXN>(sa, s_mem, cst, W, off);
                const double s = __dadd_rn(__dmul_rn(q, sd), __dmul_rn(p, mn[t]));
                mn[t] = chain_lazy(mo[t], s, c);
            }
            c = sp_block_max(prod, cst, c, tid);
            double* tm = mo; mo = mn; mn = tm;
            it++;
            chg = c;
            if (c <= sa.tol || it >= sa.max_iters) break;
        }
        __syncthreads();                                 // the maxima are read before prod is staged over

        // ---- the outputs, from the last iterate
        sp_weights(sa, mo, first, perm, Z, W, tid);
        spn_nu(a, mo, V, tid);
        __syncthreads();
        sp_agree_terms(sa, s_mem, cst, W, mn, g, tid);   // parked in the dead iterate (D <= T)
        spn_node_pass<MAXN, false>(a, s_mem, cst, V, nullptr, false, g, tid);   // the noise half's terms, parked in V
        if (sa.pi)
            for (int t = tid; t < T; t += kSpBlock) sa.pi[g * T + t] = mo[t];
        double acc = 0.0;
        for (int t0 = 0; t0 < T; t0 += 64) {
            const int t = t0 + tid;
            if (tid < 64 && t < T) {
                const double m = mo[t];
                prod[tid] = m;
                for (int i = 0; i < N; i++) {
                    const double r = sa.reward[(int64_t)i * T + t], nr = a.noise_reward[(int64_t)i * T + t];
                    prod[(1 + i) * 64 + tid] = __dmul_rn(m, __dadd_rn(__dmul_rn(q, r), __dmul_rn(p, nr)));
                    prod[(1 + N + i) * 64 + tid] = __dmul_rn(m, sa.scaled[(int64_t)i * T + t]);
                }
                prod[(1 + 2 * N) * 64 + tid] = __dmul_rn(m, __dadd_rn(__dmul_rn(q, sa.price[t]), __dmul_rn(p, a.noise_price[t])));
            }
            __syncthreads();
            acc = chain_read_back(prod, n_out, min(64, T - t0), acc, tid);
            if (tid == 64 && t0 == 0) {
                for (int d = 0; d < D; d++) acc = __dadd_rn(acc, mn[d]);
            } else if (tid == 128 && t0 == 0) {
                for (int j = 0; j < Jn; j++) acc = __dadd_rn(acc, V[j]);
                cst->red[0] = acc;
            }
            __syncthreads();
        }
        chain_store(sa.iters, sa.change, sa.mass, sa.samp_price, sa.samp_reward, sa.samp_action, g, G, N, tid, it, chg, acc);
        if (tid == 64) sa.agree[g] = __dadd_rn(__dmul_rn(q, acc), __dmul_rn(p, cst->red[0]));
    }
}

// max_jump[g] = max over the networks i, the nodes 1 <= j < Jn - 1 and the actions k of |Pn_i(k|j + 1) - Pn_i(k|j)|
__device__ __forceinline__ void spn_jump_block(const SpnArgs& a, double* red, int tid, int bid, int nblk) {
    const int N = a.sp.N, Jn = a.Jn;
    for (int64_t g = bid; g < a.sp.G; g += nblk) {
        double c = 0.0;
        for (int i = 0; i < N; i++)
            if (a.sp.kind[i] != 0) {
                const int A = a.sp.n_actions[i];
                const float* __restrict__ r = a.nprob[i] + g * Jn * A;
                const int hi = (Jn - 1) * A;             // entry e of node e / A >= 1 against the one a row further
                for (int e = A + tid; e < hi; e += kSpBlock) c = fmax(c, fabs(__dsub_rn((double)r[e + A], (double)r[e])));
            }
        red[tid] = c;
        __syncthreads();
        for (int h = kSpBlock / 2; h >= 1; h >>= 1) {
            if (tid < h) red[tid] = fmax(red[tid], red[tid + h]);
            __syncthreads();
        }
        if (tid == 0) a.max_jump[g] = red[0];
        __syncthreads();
    }
}

#ifndef THRL_SP_HOST_BUILD
template <int MAXN>
__global__ void __launch_bounds__(kSpBlock) k_spn_chain(const SpnArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    spn_block<MAXN>(a, s_mem, (int)threadIdx.x, (int)blockIdx.x, (int)gridDim.x);
}

__global__ void __launch_bounds__(kSpBlock) k_spn_jump(const SpnArgs a) {
    __shared__ double red[kSpBlock];
    spn_jump_block(a, red, (int)threadIdx.x, (int)blockIdx.x, (int)gridDim.x);
}
#endif

}  // namespace

#ifndef THRL_SP_HOST_BUILD
int launch_sampled_noise_chain(const SpnArgs& a, int grid, hipStream_t s) {
    if (a.max_jump) {
        const int jg = a.sp.G < 4096 ? a.sp.G : 4096;
        hipLaunchKernelGGL(k_spn_jump, dim3(jg), dim3(kSpBlock), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return sp_launch(k_spn_chain<2>, k_spn_chain<kSpMaxA>, a, a.sp, grid, s);
}
#endif

}  // namespace thrl
