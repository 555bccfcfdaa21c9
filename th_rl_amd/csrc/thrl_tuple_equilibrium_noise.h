// thrl_tuple_equilibrium_noise.h -- launch arguments of the equilibrium check under demand noise in tuple form
// (thrl_tuple_equilibrium_noise, include/thrl.h).  thrl_api_analysis.hip validates, ten_layout() lays out LDS;
// thrl_tuple_equilibrium_noise.hip holds the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thrl_device.h"

namespace thrl {

constexpr int kTenMaxBlocksPerCu = 32;         // one-wave blocks
constexpr int kTenSums = 4;                    // staged terms: loss, w * loss, w * [differs], w * V_pi

struct TenArgs {
    int32_t G, N, T, J, W;
    int32_t agents;
    int32_t max_sweeps;
    int32_t lds_bytes;
    // byte offsets into the block's LDS
    int32_t o_va, o_vb, o_vpi, o_x, o_rt, o_prod, o_tup, o_tcur;
    double noise_prob, eval_tol;
    double gamma[THRL_MAXA];
    int32_t n_actions[THRL_MAXA];
    int32_t tstride[THRL_MAXA];                // prod_{j > i} n_actions[j]: agent 0 slowest
    const double* noise_prob_g;                // [G] or NULL
    const double* sweep_gamma;                 // [N][G] or NULL
    const uint16_t* tuple_policy;              // [G][N][T]
    const uint16_t* cell_policy;               // [G][N][J]
    const double* reward;                      // [N][T]
    const int32_t* band_lo;                    // [T]
    const double* band;                        // [T][W]
    const double* noise_reward;                // [N][T]
    const double* pi;                          // [G][T] or NULL
    int32_t *iters, *sweeps, *n_diff_tuples, *n_diff_cells;          // [N][G]
    double *loss_all, *loss_tuples_mean, *loss_cells_mean, *loss_w, *diff_w, *v_w;
    uint16_t* br_policy;                       // [N][G][T + J] or NULL
    double *v_opt, *v_pi;
};

// LDS of a block (the working set of include/thrl.h), S = T + J: three value arrays over the states, the value and the
// expected reward per tuple, the staging of the ordered sums, then the incumbent's and the current strategy's tuple per
// state.  Returns the bytes: 44 T + 28 J + 2048, rounded up to 16.
inline int64_t ten_layout(TenArgs& a) {
    const int64_t T = a.T, S = (int64_t)a.T + a.J;
    int64_t off = 0;
    a.o_va = (int32_t)off; off += 8 * S;
    a.o_vb = (int32_t)off; off += 8 * S;
    a.o_vpi = (int32_t)off; off += 8 * S;
    a.o_x = (int32_t)off; off += 8 * T;
    a.o_rt = (int32_t)off; off += 8 * T;
    a.o_prod = (int32_t)off; off += 8 * 64 * kTenSums;
    a.o_tup = (int32_t)off; off += 2 * S;
    a.o_tcur = (int32_t)off; off += 2 * S;
    off = (off + 15) & ~(int64_t)15;
    a.lds_bytes = (int32_t)off;
    return off;
}

int launch_tuple_equilibrium_noise(const TenArgs& a, int grid, hipStream_t s);

}  // namespace thrl
