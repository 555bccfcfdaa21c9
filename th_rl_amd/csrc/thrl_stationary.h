// thrl_stationary.h -- launch arguments of the stationary-distribution kernel (thrl_stationary, include/thrl.h).
// thrl_api_analysis.hip validates and takes the per-config plan of thrl_equilibrium (the rewards per tuple) from its
// cache, stat_layout() lays out LDS; thrl_stationary.hip holds the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thrl_device.h"

namespace thrl {

constexpr int kStatLdsBudget = 64 * 1024;      // per one-wave block; the per-cell det / band tables stay in global memory
                                               // if they do not fit beside the two iterates
constexpr int kStatMaxBlocksPerCu = 32;

struct StatArgs {
    int32_t G, N, T, P, J, W;
    int32_t max_iters;
    int32_t start_state;                       // mu_0 = the unit mass on state0's cell (else cell_w)
    int32_t cell_lds;                          // det / band_lo / band offset per cell are staged in LDS
    int32_t lds_bytes;
    // byte offsets into the block's LDS
    int32_t o_mua, o_mub, o_prod, o_boff, o_blo, o_det, o_tup;
    double noise_prob, tol;
    EnvParams env;
    AgentParams ag[THRL_MAXA];
    int32_t tstride[THRL_MAXA];                // tuple index = sum_i a_i * tstride[i] (agent 0 slowest)
    int32_t row_off[THRL_MAXA];                // first policy entry of agent i in a game's P entries
    const uint16_t* policy;                    // [G][P]
    const double* noise_prob_g;                // [G] or NULL
    const double* state0;                      // [G] (start_state)
    const double* rew;                         // plan, device: [N][T] reward of agent i at tuple t
    const int32_t* cell_rows;                  // [N][J]
    const double* cell_w;                      // [J]
    const int32_t* det_cell;                   // [T]
    const int32_t* band_lo;                    // [T]
    const double* band;                        // [T][W]
    const double* noise_reward;                // [N][T]
    const double* noise_price;                 // [T]
    int32_t* iters;
    double *change, *mass, *stat_reward, *stat_action, *stat_price, *pi;
};

// LDS of a block, from N and J: 8-byte arrays first, then 4-byte, then 2-byte.  Returns the bytes without the per-cell
// tables (the two iterates, the staging of the ordered sums, the tuple per cell: refused over the budget).
inline int64_t stat_layout(StatArgs& a) {
    const int N = a.N;
    const int64_t J = a.J;
    const int64_t need = 8 * 2 * J + 8 * 64 * (int64_t)(2 * N + 2) + 2 * J + 16;
    a.cell_lds = need + 10 * J <= kStatLdsBudget;
    int off = 0;
    a.o_mua = off; off += 8 * a.J;
    a.o_mub = off; off += 8 * a.J;
    a.o_prod = off; off += 8 * 64 * (2 * N + 2);
    a.o_boff = off; off += a.cell_lds ? 4 * a.J : 0;
    a.o_blo = off; off += a.cell_lds ? 4 * a.J : 0;
    a.o_det = off; off += a.cell_lds ? 2 * a.J : 0;
    a.o_tup = off; off += 2 * a.J;
    a.lds_bytes = (off + 15) & ~15;
    return need;
}

int launch_stationary(const StatArgs& a, int grid, hipStream_t s);

}  // namespace thrl
