// thrl_sampled.h -- launch arguments of sampled play (thrl_sampled_chain, include/thrl.h).  thrl_api_analysis.hip validates;
// sp_layout() is the one place the LDS layout is written down; thrl_sampled.hip holds the kernel.  Also what the four
// calls on sampled play share on the host: the head of the two response layouts (sr_layout_head) and the launch of a
// block kernel in its <2> or <kSpMaxA> form (sp_launch).
#pragma once
#ifndef THRL_SP_HOST_BUILD
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#ifndef THRL_SP_HOST_BUILD
#include "thrl_device.h"
#endif

namespace thrl {

constexpr int kSpBlock = 256;                  // threads of a game's block
constexpr int kSpMaxBlocksPerCu = 8;
constexpr int kSpMaxA = 8;                     // THRL_MAXA

struct SpArgs {
    int32_t G, N, T, D;
    int32_t max_iters;
    int32_t start_tuple;                       // m_0 = the unit mass on start[g] (else 1 / T everywhere)
    int32_t lds_bytes;
    // byte offsets into the block's LDS (each array starts on a multiple of 16)
    int32_t o_ma, o_mb, o_w, o_z, o_first, o_perm, o_prod, o_cst;
    int32_t o_row[kSpMaxA];                    // agent i's rows: float [D][A_i] (network) or uint16 [D] (QTable)
    int32_t kind[kSpMaxA];                     // 0 = QTable, 1 / 2 = network
    int32_t n_actions[kSpMaxA];
    int32_t tstride[kSpMaxA];                  // prod_{j > i} n_actions[j]: agent 0 slowest
    double eps[kSpMaxA];
    double tol;
    const double* eps_g;                       // [N][G] or NULL
    const int32_t* start;                      // [G] (start_tuple)
    const float* prob[kSpMaxA];                // [G][D][A_i] (networks)
    const uint16_t* dpolicy;                   // [G][N][D]
    const int32_t* grp_first;                  // [D + 1]
    const int32_t* grp_perm;                   // [T]
    const double* reward;                      // [N][T]
    const double* scaled;                      // [N][T]
    const double* price;                       // [T]
    int32_t* iters;
    double *change, *mass, *samp_reward, *samp_action, *samp_price, *agree, *pi;
};

inline int64_t r16(int64_t x) { return (x + 15) & ~(int64_t)15; }   // every LDS array starts on a multiple of 16

// the LDS layout of include/thrl.h's working set; returns the bytes of a block
inline int32_t sp_layout(SpArgs& a) {
    int64_t off = 0;
    a.o_ma = (int32_t)off; off += r16(8 * (int64_t)a.T);
    a.o_mb = (int32_t)off; off += r16(8 * (int64_t)a.T);
    a.o_w = (int32_t)off; off += r16(8 * (int64_t)a.D);
    a.o_z = (int32_t)off; off += r16(8 * (int64_t)a.D);
    for (int i = 0; i < a.N; i++) {
        a.o_row[i] = (int32_t)off;
        off += r16(a.kind[i] == 0 ? 2 * (int64_t)a.D : 4 * (int64_t)a.D * a.n_actions[i]);
    }
    a.o_first = (int32_t)off; off += r16(2 * ((int64_t)a.D + 1));
    a.o_perm = (int32_t)off; off += r16(2 * (int64_t)a.T);
    a.o_prod = (int32_t)off; off += r16(512 * (2 * (int64_t)a.N + 2));
    a.o_cst = (int32_t)off; off += 256;
    a.lds_bytes = (int32_t)off;
    return a.lds_bytes;
}

// The head of sr_layout and srn_layout (Args = SrArgs, SrnArgs) over S states: five arrays of 8 S (o_va, o_vb, o_vpi, o_zm,
// o_si), two of 8 T (o_u, o_rt), the agents' rows at the D prices, first, perm, trow, and sigma and modal of 2 S.  Returns
// the offset behind them, where each layout's own tail begins.
template <typename Args>
inline int64_t sr_layout_head(Args& a, int64_t S) {
    const int64_t T = a.sp.T, D = a.sp.D;
    int64_t off = 0;
    a.o_va = (int32_t)off; off += r16(8 * S);
    a.o_vb = (int32_t)off; off += r16(8 * S);
    a.o_vpi = (int32_t)off; off += r16(8 * S);
    a.o_zm = (int32_t)off; off += r16(8 * S);
    a.o_si = (int32_t)off; off += r16(8 * S);
    a.o_u = (int32_t)off; off += r16(8 * T);
    a.o_rt = (int32_t)off; off += r16(8 * T);
    for (int i = 0; i < a.sp.N; i++) {
        a.sp.o_row[i] = (int32_t)off;
        off += r16(a.sp.kind[i] == 0 ? 2 * D : 4 * D * a.sp.n_actions[i]);
    }
    a.sp.o_first = (int32_t)off; off += r16(2 * (D + 1));
    a.sp.o_perm = (int32_t)off; off += r16(2 * T);
    a.o_trow = (int32_t)off; off += r16(2 * T);
    a.o_sigma = (int32_t)off; off += r16(2 * S);
    a.o_modal = (int32_t)off; off += r16(2 * S);
    return off;
}

#ifndef THRL_SP_HOST_BUILD
int launch_sampled_chain(const SpArgs& a, int grid, hipStream_t s);

// Launches a block kernel of sampled play on `grid` blocks of kSpBlock threads with sp.lds_bytes of dynamic LDS: k2 with
// two agents, k8 with more.  Above 64 KB the kernel is first allowed that much.  Returns the HIP error, 0 for none.
template <typename Args>
inline int sp_launch(void (*k2)(const Args), void (*k8)(const Args), const Args& a, const SpArgs& sp, int grid, hipStream_t s) {
    void (*const k)(const Args) = sp.N <= 2 ? k2 : k8;
    if (sp.lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 sp.lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k, dim3(grid), dim3(kSpBlock), (size_t)sp.lds_bytes, s, a);
    return (int)hipGetLastError();
}
#endif

}  // namespace thrl
