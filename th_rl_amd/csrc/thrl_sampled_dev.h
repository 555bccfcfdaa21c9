// thrl_sampled_dev.h -- the device functions k_sp_chain (thrl_sampled.hip) and k_spn_chain (thrl_sampled_noise.hip)
// share: the per-game constants, the staging of the distinct-price rows with their normaliser Z(d), the M / W pass, the
// ordered sum over the distinct prices for one output tuple and the block's maximum.  The two response kernels
// (k_sr_response, k_srn_response) take the constants, the epsilon check, the game's staging and the maximum from here;
// what those two share beyond that is thrl_response_dev.h's, and the launch of all four is thrl_sampled.h's sp_launch.
// What all four chain kernels share
// (the unsolved outputs, the lazy update, the read-back and the final store) is thrl_chain_dev.h's.  Everything sits in namespace thrl's
// anonymous namespace, once per including file; with THRL_SP_HOST_BUILD the host harness supplies __device__, __syncthreads() and
// the rounded operations.
#pragma once
#include "thrl_sampled.h"
#include "thrl_chain_dev.h"

namespace thrl {

namespace {

struct SpCst {                                   // per game, per QTable agent: eps / A and (1 - eps) + eps / A
    double lo[kSpMaxA], hi[kSpMaxA];
    double red[16];                              // the second level of the maximum
};

// M(d) over the tuples of price d in ascending t, W(d) = M(d) / Z(d)
__device__ __forceinline__ void sp_weights(const SpArgs& a, const double* m, const uint16_t* first, const uint16_t* perm,
                                           const double* Z, double* W, int tid) {
    for (int d = tid; d < a.D; d += kSpBlock) {
        double M = 0.0;
        const int e = first[d + 1];
        for (int s = first[d]; s < e; s++) M = __dadd_rn(M, m[perm[s]]);
        W[d] = __ddiv_rn(M, Z[d]);
    }
}

// a QTable agent's epsilon of game g lies in [0, 1] (a network's is not read)
__device__ __forceinline__ bool sp_eps_ok(const SpArgs& a, int64_t g) {
    bool ok = true;
    for (int i = 0; i < a.N; i++)
        if (a.kind[i] == 0) {
            const double e = a.eps_g ? a.eps_g[(int64_t)i * a.G + g] : a.eps[i];
            ok = ok && e >= 0.0 && e <= 1.0;
        }
    return ok;
}

// the game's constants and its rows at the distinct prices; the caller synchronises before it reads them.  UNROLL is the
// QTable rows' copy's: it runs once per game, but its registers count.  k_sp_chain keeps it rolled (the compiler's own
// choice costs it six registers and a wave per SIMD); k_spn_chain<8>, which has none to spare, takes scratch unless it is 2
template <int UNROLL>
__device__ __forceinline__ void sp_stage_game(const SpArgs& a, unsigned char* s_mem, SpCst* cst, int64_t g, int tid) {
    const int N = a.N, G = a.G, D = a.D;
    if (tid < N) {
        double lo = 0.0, hi = 0.0;
        if (a.kind[tid] == 0) {
            const double e = a.eps_g ? a.eps_g[(int64_t)tid * G + g] : a.eps[tid];
            lo = __ddiv_rn(e, (double)a.n_actions[tid]);
            hi = __dadd_rn(__dsub_rn(1.0, e), lo);
        }
        cst->lo[tid] = lo;
        cst->hi[tid] = hi;
    }
    for (int i = 0; i < N; i++) {
        const int A = a.n_actions[i];
        if (a.kind[i] == 0) {
            uint16_t* rq = reinterpret_cast<uint16_t*>(s_mem + a.o_row[i]);
            const uint16_t* __restrict__ src = a.dpolicy + (g * N + i) * D;
#pragma unroll UNROLL
            for (int d = tid; d < D; d += kSpBlock) rq[d] = (uint16_t)min((int)src[d], A - 1);
        } else {
            float* rf = reinterpret_cast<float*>(s_mem + a.o_row[i]);
            const int n = D * A;
            const float* __restrict__ src = a.prob[i] + g * n;
            for (int j = tid; j < n; j += kSpBlock) rf[j] = src[j];
        }
    }
}

// Z(d) = S_0(d) * S_1(d) * ... from the staged rows
__device__ __forceinline__ void sp_normaliser(const SpArgs& a, const unsigned char* s_mem, double* Z, int tid) {
    for (int d = tid; d < a.D; d += kSpBlock) {
        double z = 1.0;
        for (int i = 0; i < a.N; i++) {
            double S = 1.0;
            if (a.kind[i] != 0) {
                const int A = a.n_actions[i];
                const float* rf = reinterpret_cast<const float*>(s_mem + a.o_row[i]) + d * A;
                S = 0.0;
                for (int k = 0; k < A; k++) S = __dadd_rn(S, (double)rf[k]);
            }
            z = i == 0 ? S : __dmul_rn(z, S);
        }
        Z[d] = z;
    }
}

// where tuple t's action sits in a row of agent i
template <int MAXN>
__device__ __forceinline__ void sp_offsets(const SpArgs& a, int t, int (&off)[MAXN]) {
#pragma unroll
    for (int i = 0; i < MAXN; i++) off[i] = i < a.N ? (t / a.tstride[i]) % a.n_actions[i] : 0;
}

// sum_d ((W(d) * P_0(a_0|d)) * P_1(a_1|d)) * ... in ascending d from 0.0 for the tuple with the offsets `off`
template <int MAXN>
__device__ __forceinline__ double sp_price_sum(const SpArgs& a, const unsigned char* s_mem, const SpCst* cst, const double* W,
                                               const int (&off)[MAXN]) {
    const int N = a.N, D = a.D;
    double s = 0.0;
    for (int d = 0; d < D; d++) {
        const double w = W[d];
        if (w == 0.0) continue;                  // no mass at this price: the terms are +0.0
        double term = w;
#pragma unroll
        for (int i = 0; i < MAXN; i++) {
            if (i >= N) break;
            double p;
            if (a.kind[i] == 0) {
                const uint16_t* rq = reinterpret_cast<const uint16_t*>(s_mem + a.o_row[i]);
                p = (int)rq[d] == off[i] ? cst->hi[i] : cst->lo[i];
            } else {
                const float* rf = reinterpret_cast<const float*>(s_mem + a.o_row[i]);
                p = (double)rf[d * a.n_actions[i] + off[i]];
            }
            term = __dmul_rn(term, p);
        }
        s = __dadd_rn(s, term);
    }
    return s;
}

// the block's maximum of c through LDS in two levels, no shuffle (the order of a maximum is free)
__device__ __forceinline__ double sp_block_max(double* prod, SpCst* cst, double c, int tid) {
    prod[tid] = c;
    __syncthreads();
    if (tid < 16) {
        double cc = prod[tid * 16];
        for (int k = 1; k < 16; k++) cc = fmax(cc, prod[tid * 16 + k]);
        cst->red[tid] = cc;
    }
    __syncthreads();
    c = cst->red[0];
    for (int k = 1; k < 16; k++) c = fmax(c, cst->red[k]);
    return c;
}

// agree's terms at the distinct prices, parked in out[0 .. D)
__device__ __forceinline__ void sp_agree_terms(const SpArgs& a, const unsigned char* s_mem, const SpCst* cst, const double* W,
                                               double* out, int64_t g, int tid) {
    const int N = a.N, D = a.D;
    for (int d = tid; d < D; d += kSpBlock) {
        double term = W[d];
        for (int i = 0; i < N; i++) {
            const int A = a.n_actions[i];
            double p;
            if (a.kind[i] == 0) {
                p = cst->hi[i];
            } else {
                const int gi = min((int)a.dpolicy[(g * N + i) * D + d], A - 1);
                p = (double)(reinterpret_cast<const float*>(s_mem + a.o_row[i])[d * A + gi]);
            }
            term = __dmul_rn(term, p);
        }
        out[d] = term;
    }
}

}  // namespace

}  // namespace thrl
