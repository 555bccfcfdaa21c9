// thrl_deviation.h -- launch arguments of the deviation-analysis kernel (thrl_deviation, include/thrl.h).
// thrl_api_analysis.hip validates and plans; thrl_deviation.hip holds the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thrl_device.h"

namespace thrl {

constexpr int kDevTile = 256;                  // games per block, one lane per game
constexpr int kDevLdsBudget = 64 * 1024;       // staged policy + scale LUT per block; larger configs read rows from HBM
constexpr int kDevMaxLut = 1024;               // sum of the agents' action counts the staged path's scale LUT holds

struct DevArgs {
    int32_t G, N, d, L, K, H, dev_action, row_begin, row_count;
    int32_t staged;                            // 1: policy staged in LDS (1 or 2 bytes per entry), 0: direct
    int32_t pol_bytes;                         // 1 or 2 (staged)
    int32_t pol_entries;                       // entries per game: sum_i (win_n[i] + 1)
    int32_t lds_bytes;
    int32_t lut_n;                             // sum_i n_actions[i]: entries of the staged scale LUT
    int64_t stride;
    EnvParams env;
    AgentParams ag[THRL_MAXA];
    int32_t win_lo[THRL_MAXA], win_n[THRL_MAXA], pol_off[THRL_MAXA + 1], lut_off[THRL_MAXA];
    const void* q;
    const double* state0;
    const double* sweep_gamma;
    int32_t *mu, *lam, *mu_post, *lam_post, *ret_step, *act_dev;
    double *cycle_reward, *cycle_action, *gain;
    double *reward_rows, *action_rows;
};

int launch_deviation(const DevArgs& a, int q_dtype, hipStream_t s);

}  // namespace thrl
