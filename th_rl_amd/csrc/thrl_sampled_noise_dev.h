// thrl_sampled_noise_dev.h -- the node half of sampled play under demand noise, the device functions k_spn_chain
// (thrl_sampled_noise.hip) and k_sdn_chain (thrl_sampled_deviation_noise.hip) share: the streamed, double-buffered,
// register-staged tiles of the networks' node rows (spn_lead, spn_tile_load, spn_tile_store, spn_tile_rows), nu (spn_nu)
// and the walk over the nodes in ascending j (spn_node_pass).  `det` names an agent that is deterministic for this pass
// whatever its kind (k_sdn_chain's deviator while the deviation lasts): its node entries are the uint16 row det_row,
// its probabilities 1.0 / 0.0 and its row sum 1.0 exactly; a network's tile is then neither loaded nor read.  -1, the
// default, is nobody, and the functions compile to what they were without the switch.  Everything sits in namespace
// thrl's anonymous namespace, once per including file; with THRL_SP_HOST_BUILD the host harness supplies __device__,
// __syncthreads() and the rounded operations.
#pragma once
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
__device__ __forceinline__ void spn_tile_load(const SpnArgs& a, int64_t g, int j0, int tid, SpnWord (&st)[MAXN][kSpnChunks],
                                              int det = -1) {
    const int n = min(kSpnTile, a.Jn - j0);
#pragma unroll
    for (int i = 0; i < MAXN; i++) {
        if (i < a.sp.N && a.sp.kind[i] != 0 && i != det) {
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
                                               const SpnWord (&st)[MAXN][kSpnChunks], int det = -1) {
    const int n = min(kSpnTile, a.Jn - j0);
#pragma unroll
    for (int i = 0; i < MAXN; i++) {
        if (i < a.sp.N && a.sp.kind[i] != 0 && i != det) {
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
// ((V(j) * Pn_0(gn_0(j)|j)) * ...).  With det >= 0 (ACC only) agent det plays
// det_row[j] at node j: probability 1.0 there and 0.0 elsewhere, Sn_det = 1.0.  Ends on a barrier.
template <int MAXN, bool ACC>
__device__ __forceinline__ void spn_node_pass(const SpnArgs& a, unsigned char* s_mem, const SpCst* cst, double* V, double* acc,
                                              bool reset, int64_t g, int tid, int det = -1, const uint16_t* det_row = nullptr) {
    const int N = a.sp.N, T = a.sp.T, Jn = a.Jn;
    const int n_tiles = (Jn + kSpnTile - 1) / kSpnTile;
    SpnWord st[MAXN][kSpnChunks];
    spn_tile_load<MAXN>(a, g, 0, tid, st, det);
    spn_tile_store<MAXN>(a, s_mem, 0, g, 0, tid, st, det);
    __syncthreads();
    for (int k = 0; k < n_tiles; k++) {
        const int j0 = k * kSpnTile, n = min(kSpnTile, Jn - j0), buf = k & 1;
        if (k + 1 < n_tiles) spn_tile_load<MAXN>(a, g, j0 + kSpnTile, tid, st, det);
        if (tid < n) {                                           // V of the tile's nodes, one lane per node
            const int j = j0 + tid;
            double z = 1.0;
            for (int i = 0; i < N; i++) {
                double S = 1.0;
                if (a.sp.kind[i] != 0 && i != det) {
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
                        if (i == det) {
                            p = (int)det_row[j0 + jj] == off[i] ? 1.0 : 0.0;
                        } else if (a.sp.kind[i] == 0) {
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
        if (k + 1 < n_tiles) spn_tile_store<MAXN>(a, s_mem, buf ^ 1, g, j0 + kSpnTile, tid, st, det);
        __syncthreads();
    }
}

}  // namespace

}  // namespace thrl
