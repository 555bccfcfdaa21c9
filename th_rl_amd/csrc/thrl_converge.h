// thrl_converge.h -- launch arguments of the convergence-tracking kernel (thrl_policy_track, include/thrl.h).
// thrl_api_analysis.hip validates and plans; thrl_converge.hip holds the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thrl_device.h"

namespace thrl {

constexpr int kTrackLdsBudget = 64 * 1024;     // staged window of one game's tables; larger configs read from HBM
constexpr int kTrackMaxBlocksPerCu = 16;

struct TrackArgs {
    int32_t G, N, P;                           // games, agents, policy entries per game
    int32_t baseline;                          // THRL_TRACK_BASELINE
    int32_t staged;                            // 1: the game's tables staged in LDS with 16-byte loads, 0: direct
    int32_t lds_bytes;
    int64_t stride;                            // elements per game
    int64_t episode, window;
    int32_t row_off[THRL_MAXA + 1];            // first policy entry of agent i; row_off[N] = P
    int32_t table_off[THRL_MAXA];              // element offset of agent i's table in a game's block
    int32_t n_actions[THRL_MAXA];
    const void* q;
    uint16_t* policy;
    int64_t *stable_since, *converged_at, *conv_since;
    int32_t *changes, *n_converged;
    const double* state;
    void* q_conv;
    double* state_conv;
};

// grid: blocks of one wavefront, each looping over games blockIdx.x, + gridDim.x, ...
int launch_policy_track(const TrackArgs& a, int q_dtype, int grid, hipStream_t s);

}  // namespace thrl
