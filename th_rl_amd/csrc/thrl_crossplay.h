// thrl_crossplay.h -- launch arguments of the cross-play kernels (thrl_crossplay, include/thrl.h).
// thrl_api_analysis.hip validates and plans; thrl_crossplay.hip holds the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thrl_deviation.h"
#include "thrl_device.h"

namespace thrl {

constexpr int kXpTile = 256;                   // matches per block of the walk, one lane per match
constexpr int kXpLdsBudget = 64 * 1024;        // walk: staged windows + scale LUT per block; larger configs gather from global
constexpr int kXpExtractLdsBudget = 64 * 1024; // extraction: staged window of one game's tables; larger configs read from HBM
constexpr int kXpExtractMaxBlocksPerCu = 16;

struct XpExtractArgs {
    int32_t G, N, P;                           // games, agents, policy entries per game
    int32_t staged;                            // 1: the game's tables staged in LDS with 16-byte loads, 0: direct
    int32_t lds_bytes;
    int64_t stride;                            // elements per game
    int32_t row_off[THRL_MAXA + 1];            // first policy entry of agent i; row_off[N] = P
    int32_t table_off[THRL_MAXA];              // element offset of agent i's table in a game's block
    int32_t n_actions[THRL_MAXA];
    const void* q;
    uint16_t* policy;
};

struct XpWalkArgs {
    int32_t G, M, N, P, H, K, row_begin, row_count;
    int32_t staged;                            // 1: every match's policy windows staged in LDS, 0: gathered from global
    int32_t use_lut;                           // 1: scaled actions from an LDS table of lut_n entries
    int32_t pol_entries;                       // staged entries per match: sum_i (win_n[i] + 1)
    int32_t lds_bytes;
    int32_t lut_n;                             // sum_i n_actions[i]
    EnvParams env;
    AgentParams ag[THRL_MAXA];
    int32_t row_off[THRL_MAXA];                // first policy entry of agent i in a game's P entries
    int32_t win_lo[THRL_MAXA], win_n[THRL_MAXA], pol_off[THRL_MAXA + 1], lut_off[THRL_MAXA];
    const uint16_t* policy;
    const int32_t* seat;
    const double* state0;
    int32_t *mu, *lam;
    double *cycle_reward, *cycle_action;
    double *reward_rows, *action_rows;
};

// grid: blocks of one wavefront, each looping over games blockIdx.x, + gridDim.x, ...
int launch_xplay_extract(const XpExtractArgs& a, int q_dtype, int grid, hipStream_t s);
int launch_xplay_walk(const XpWalkArgs& a, hipStream_t s);

}  // namespace thrl
