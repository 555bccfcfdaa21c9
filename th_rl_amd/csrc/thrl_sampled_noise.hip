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
// k_spn_jump: max_jump, the largest change of a network's probability between adjacent nodes, for every game.
//   Nothing in the bodies is wave-specific: with THRL_SP_HOST_BUILD the same source runs as 256 host threads with barriers.
#include "thrl_sampled_noise.h"
#include "thrl_sampled_dev.h"

namespace thrl {

namespace {

#ifdef THRL_SP_HOST_BUILD
#define THRL_SPN_WAVE_FIRST(x, tid) ((x) - ((tid) & 63))
#else
#define THRL_SPN_WAVE_FIRST(x, tid) __builtin_amdgcn_readfirstlane(x)
#endif

struct alignas(16) SpnWord { float f[4]; };

// floats between the 16-byte boundary below a tile's first row and that row
__device__ __forceinline__ int spn_lead(const float* src) { return (int)((reinterpret_cast<uintptr_t>(src) & 15) >> 2); }

// the rows of the nodes [j0, j0 + n) of every network, into registers
template <int MAXN>
__device__ __forceinline__ void spn_tile_load(const SpnArgs& a, int64_t g, int j0, int tid, SpnWord (&st)[MAXN][kSpnChunks]) {
    const int n = min(kSpnTile, a.Jn - j0);
#pragma unroll
    for (int i = 0; i < MAXN; i++) {
        if (i < a.sp.N && a.sp.kind[i] != 0) {
            const int A = a.sp.n_actions[i];
            const float* __restrict__ src = a.nprob[i] + (g * a.Jn + j0) * A;
            const int lead = spn_lead(src), nf = n * A;
            const SpnWord* __restrict__ base = reinterpret_cast<const SpnWord*>(src - lead);
#pragma unroll
            for (int c = 0; c < kSpnChunks; c++) {
                const int w = c * kSpBlock + tid;
                const int e0 = 4 * w - lead;                     // the word holds floats [e0, e0 + 4) of the tile
                SpnWord v = {{0.0f, 0.0f, 0.0f, 0.0f}};
                if (e0 >= 0 && e0 + 4 <= nf) {
                    v = base[w];
                } else {
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if ((uint32_t)(e0 + q) < (uint32_t)nf) v.f[q] = src[e0 + q];
                }
                st[i][c] = v;
            }
        }
    }
}

template <int MAXN>
__device__ __forceinline__ void spn_tile_store(const SpnArgs& a, unsigned char* s_mem, int buf, int64_t g, int j0, int tid,
                                               const SpnWord (&st)[MAXN][kSpnChunks]) {
    const int n = min(kSpnTile, a.Jn - j0);
#pragma unroll
    for (int i = 0; i < MAXN; i++) {
        if (i < a.sp.N && a.sp.kind[i] != 0) {
            const int A = a.sp.n_actions[i];
            const int lead = spn_lead(a.nprob[i] + (g * a.Jn + j0) * A), nf = n * A;
            SpnWord* dst = reinterpret_cast<SpnWord*>(s_mem + a.o_tile[i][buf]);
#pragma unroll
            for (int c = 0; c < kSpnChunks; c++) {
                const int w = c * kSpBlock + tid;
                if (4 * w - lead < nf) dst[w] = st[i][c];        // w <= (kSpnTile A + 2) / 4: inside the buffer
            }
        }
    }
}

// network i's rows of the tile resident in `buf`: row jj at [jj * A_i]
__device__ __forceinline__ const float* spn_tile_rows(const SpnArgs& a, const unsigned char* s_mem, int i, int buf, int64_t g, int j0) {
    return reinterpret_cast<const float*>(s_mem + a.o_tile[i][buf])
        + spn_lead(a.nprob[i] + (g * a.Jn + j0) * a.sp.n_actions[i]);
}

// nu(j) = sum_t m(t) nn(t, j) in ascending t, left in V[j]
__device__ __forceinline__ void spn_nu(const SpnArgs& a, const double* m, double* V, int tid) {
    const int T = a.sp.T, Jn = a.Jn, W = a.W;
    for (int k0 = tid; k0 < Jn; k0 += 2 * kSpBlock) {
        const int k1 = k0 + kSpBlock;
        const int kw = THRL_SPN_WAVE_FIRST(k0, tid);             // the wave's nodes: [kw, kw + 64) and 256 further
        double s0 = 0.0, s1 = 0.0;
        for (int t = 0; t < T; t++) {
            const double mt = m[t];
            if (mt == 0.0) continue;                             // the terms are +0.0: adding them changes nothing
            const int blo = a.band_lo[t];
            if (blo >= kw + kSpBlock + 64 || (int64_t)blo + W <= kw) continue;
            const uint32_t d0 = (uint32_t)(k0 - blo), d1 = (uint32_t)(k1 - blo);
            const double* __restrict__ row = a.band + (int64_t)t * W;
            const double n0 = d0 < (uint32_t)W ? row[d0] : 0.0;
            const double n1 = (d1 < (uint32_t)W && k1 < Jn) ? row[d1] : 0.0;
            if (n0 != 0.0) s0 = __dadd_rn(s0, __dmul_rn(mt, n0));
            if (n1 != 0.0) s1 = __dadd_rn(s1, __dmul_rn(mt, n1));
        }
        V[k0] = s0;
        if (k1 < Jn) V[k1] = s1;
    }
}

// One walk over the nodes in ascending j, tile by tile.  V holds the numerators (nu, or node_w with `reset`, where a
// zero weight gives V = 0); as a tile is resident V(j) = numerator / Zn(j) replaces them.  ACC: acc[t'] = sum_j ((V(j) *
// Pn_0(a_0(t')|j)) * Pn_1(a_1(t')|j)) * ..., a j with V(j) == 0.0 skipped.  Otherwise V[j] becomes agree's term
// ((V(j) * Pn_0(gn_0(j)|j)) * ...).  Ends on a barrier.
template <int MAXN, bool ACC>
__device__ __forceinline__ void spn_node_pass(const SpnArgs& a, unsigned char* s_mem, const SpCst* cst, double* V, double* acc,
                                              bool reset, int64_t g, int tid) {
    const int N = a.sp.N, T = a.sp.T, Jn = a.Jn;
    const int n_tiles = (Jn + kSpnTile - 1) / kSpnTile;
    SpnWord st[MAXN][kSpnChunks];
    spn_tile_load<MAXN>(a, g, 0, tid, st);
    spn_tile_store<MAXN>(a, s_mem, 0, g, 0, tid, st);
    __syncthreads();
    for (int k = 0; k < n_tiles; k++) {
        const int j0 = k * kSpnTile, n = min(kSpnTile, Jn - j0), buf = k & 1;
        if (k + 1 < n_tiles) spn_tile_load<MAXN>(a, g, j0 + kSpnTile, tid, st);
        if (tid < n) {                                           // V of the tile's nodes, one lane per node
            const int j = j0 + tid;
            double z = 1.0;
            for (int i = 0; i < N; i++) {
                double S = 1.0;
                if (a.sp.kind[i] != 0) {
                    const int A = a.sp.n_actions[i];
                    const float* rf = spn_tile_rows(a, s_mem, i, buf, g, j0) + tid * A;
                    S = 0.0;
                    for (int kk = 0; kk < A; kk++) S = __dadd_rn(S, (double)rf[kk]);
                }
                z = i == 0 ? S : __dmul_rn(z, S);
            }
            const double num = V[j];
            double v = (reset && num == 0.0) ? 0.0 : __ddiv_rn(num, z);
            if (!ACC)
                for (int i = 0; i < N; i++) {
                    double p;
                    if (a.sp.kind[i] == 0) {
                        p = cst->hi[i];
                    } else {
                        const int A = a.sp.n_actions[i];
                        const int gi = min((int)a.npolicy[(g * N + i) * Jn + j], A - 1);
                        p = (double)(spn_tile_rows(a, s_mem, i, buf, g, j0)[tid * A + gi]);
                    }
                    v = __dmul_rn(v, p);
                }
            V[j] = v;
        }
        if (ACC) {
            __syncthreads();
            for (int t = tid; t < T; t += kSpBlock) {
                int off[MAXN];
                sp_offsets<MAXN>(a.sp, t, off);
                double s = k == 0 ? 0.0 : acc[t];
                for (int jj = 0; jj < n; jj++) {
                    const double v = V[j0 + jj];
                    if (v == 0.0) continue;                      // no mass on this node: the terms are +0.0
                    double term = v;
#pragma unroll
                    for (int i = 0; i < MAXN; i++) {
                        if (i >= N) break;
                        double p;
                        if (a.sp.kind[i] == 0) {
                            const uint16_t* nq = reinterpret_cast<const uint16_t*>(s_mem + a.o_nrow[i]);
                            p = (int)nq[j0 + jj] == off[i] ? cst->hi[i] : cst->lo[i];
                        } else {
                            p = (double)spn_tile_rows(a, s_mem, i, buf, g, j0)[jj * a.sp.n_actions[i] + off[i]];
                        }
                        term = __dmul_rn(term, p);
                    }
                    s = __dadd_rn(s, term);
                }
                acc[t] = s;
            }
        }
        if (k + 1 < n_tiles) spn_tile_store<MAXN>(a, s_mem, buf ^ 1, g, j0 + kSpnTile, tid, st);
        __syncthreads();
    }
}

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
