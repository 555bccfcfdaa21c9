// thrl_tuple_play.h -- launch arguments of the tuple-policy kernels (thrl_tuple_policy, thrl_tuple_walk,
// include/thrl.h).  thrl_api_analysis.hip validates and plans; thrl_tuple_play.hip holds the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thrl_device.h"

namespace thrl {

constexpr int kTpTile = 256;                   // matches per block of the walk, one lane per match
constexpr int kTpLdsBudget = 64 * 1024;        // walk: reward and scaled tables per block; larger configs read them from global

struct TpPolicyArgs {
    int32_t G, N, T;
    int32_t n_q, n_nn;                         // QTable agents, Reinforce / ActorCritic agents
    int32_t q_agent[THRL_MAXA];                // agent index of the j-th QTable agent
    int32_t nn_agent[THRL_MAXA];               // agent index of the j-th neural agent
    int32_t nn_actions[THRL_MAXA];             // its number of actions
    int32_t nn_stride[THRL_MAXA];              // its floats per game
    const float* nn_params[THRL_MAXA];         // its parameters [G][nn_stride]
    AgentParams ag[THRL_MAXA];
    int64_t stride;                            // elements per game of q
    const void* q;
    const double* price;                       // [T], or [G][T] with price_stride = T (thrl_price_policy per game)
    int64_t price_stride;                      // doubles between two games' prices: 0 = every game reads the same T
    uint16_t* policy;                          // [G][N][T]
};

struct TpWalkArgs {
    int32_t G, M, N, T, H, K, row_begin, row_count;
    int32_t in_lds;                            // 1: reward and scaled staged in LDS (2 N T doubles)
    int32_t lds_bytes;
    int32_t n_actions[THRL_MAXA];
    int32_t tstride[THRL_MAXA];                // prod_{j > i} n_actions[j]: agent 0 slowest
    const uint16_t* policy;                    // [G][N][T]
    const int32_t* seat;                       // [N][M]
    const int32_t* start;                      // [M]
    const double* reward;                      // [N][T]
    const double* scaled;                      // [N][T]
    int32_t *mu, *lam, *cycle_start;
    double *cycle_reward, *cycle_action;
    double *reward_rows, *action_rows;
};

int launch_tp_policy(const TpPolicyArgs& a, int q_dtype, hipStream_t s);
int launch_tp_walk(const TpWalkArgs& a, hipStream_t s);
// thrl_price_probs for one neural agent: out [G][J][A], the softmax at the J shared prices
int launch_tp_probs(int G, int A, int J, const float* params, int P, const double* price, float* out, hipStream_t s);

}  // namespace thrl
