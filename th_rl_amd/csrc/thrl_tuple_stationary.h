// thrl_tuple_stationary.h -- launch arguments of the stationary analysis in tuple form (thrl_tuple_stationary,
// include/thrl.h).  thrl_api.hip validates and lays out LDS; thrl_tuple_stationary.hip holds the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thrl_device.h"

namespace thrl {

constexpr int kTsBlock = 256;                  // threads of a game's block
constexpr int kTsMaxBlocksPerCu = 8;

struct TsArgs {
    int32_t G, N, T, J, W;
    int32_t max_iters;
    int32_t start_tuple;                       // m_0 = the unit mass on start[g] (else the reset distribution)
    int32_t neural_mask;                       // bit i: agent i is a network (n_switch / unresolved)
    int32_t lds_bytes;
    // byte offsets into the block's LDS; nu follows mb directly (the sort scratch of the groupings spans both)
    int32_t o_ma, o_mb, o_nu, o_prod, o_permk, o_startk, o_permt, o_startt;
    double noise_prob, tol;
    int32_t n_actions[THRL_MAXA];
    int32_t tstride[THRL_MAXA];                // prod_{j > i} n_actions[j]: agent 0 slowest
    const double* noise_prob_g;                // [G] or NULL
    const int32_t* start;                      // [G] (start_tuple)
    const uint16_t* tuple_policy;              // [G][N][T]
    const uint16_t* cell_policy;               // [G][N][J]
    const double* cell_w;                      // [J]
    const double* reward;                      // [N][T]
    const double* scaled;                      // [N][T]
    const double* price;                       // [T]
    const int32_t* band_lo;                    // [T]
    const double* band;                        // [T][W]
    const double* noise_reward;                // [N][T]
    const double* noise_price;                 // [T]
    int32_t* iters;
    double *change, *mass, *stat_reward, *stat_action, *stat_price, *pi;
    int32_t* n_switch;
    double* unresolved;
};

int launch_tuple_stationary(const TsArgs& a, int grid, hipStream_t s);

}  // namespace thrl
