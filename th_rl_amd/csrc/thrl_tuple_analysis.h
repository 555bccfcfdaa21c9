// thrl_tuple_analysis.h -- launch arguments of the deviation test and the equilibrium check in tuple form
// (thrl_tuple_deviation, thrl_tuple_equilibrium, include/thrl.h).  thrl_api_analysis.hip validates and plans the grid,
// ta_eq_layout() lays out the equilibrium block's LDS; thrl_tuple_analysis.hip holds the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thrl_device.h"

namespace thrl {

constexpr int kTaDevTile = 256;                // deviation: games per block, one lane per game
constexpr int kTaDevLdsBudget = 64 * 1024;     // deviation: reward and scaled tables per block; larger configs read them from global
constexpr int kTaEqBlock = 256;                // equilibrium: threads of the block that solves one game
constexpr int kTaEqMaxPerLane = 16;            // THRL_TP_MAX_TUPLES / kTaEqBlock: states a lane owns at most
constexpr int kTaEqMaxBlocksPerCu = 4;         // the kernel's ~105 VGPRs leave 4 waves per SIMD: four 4-wave blocks per CU
// equilibrium, bytes of LDS per tuple: two V buffers (16), the agent's reward row (8), two jump tables (4), sigma,
// the joint map, the first-visit / changed marks and the base tuple (2 each)
constexpr int kTaEqLdsPerTuple = 36;
constexpr int kTaEqLdsFixed = 128;             // reduction scratch and the walk's results

struct TaDevArgs {
    int32_t G, N, T, H, d, L, K, dev_action, row_begin, row_count;
    int32_t in_lds;                            // 1: reward and scaled staged in LDS (2 N T doubles)
    int32_t lds_bytes;
    int32_t n_actions[THRL_MAXA];
    int32_t tstride[THRL_MAXA];                // prod_{j > i} n_actions[j]: agent 0 slowest
    double gamma_d;                            // cfg.gamma[d]
    const int32_t* start;                      // [G]
    const uint16_t* policy;                    // [G][N][T]
    const double* reward;                      // [N][T]
    const double* scaled;                      // [N][T]
    const double* sweep_gamma;                 // [N][G] or null
    int32_t *mu, *lam, *mu_post, *lam_post, *ret_step, *act_dev;
    double *cycle_reward, *cycle_action, *gain, *reward_rows, *action_rows;
};

struct TaEqArgs {
    int32_t G, N, T, agents;
    int32_t lds_bytes;
    // byte offsets into the block's LDS
    int32_t o_va, o_vb, o_rew, o_na, o_nb, o_sigma, o_jn, o_mark, o_base, o_misc;
    int32_t n_actions[THRL_MAXA];
    int32_t tstride[THRL_MAXA];
    double gamma[THRL_MAXA];                   // cfg.gamma
    const int32_t* start;
    const uint16_t* policy;
    const double* reward;
    const double* sweep_gamma;
    int32_t *mu, *lam, *iters, *n_diff_all, *n_diff_on;
    double *loss_all, *loss_on, *loss_all_mean, *loss_on_mean, *v_on;
    uint16_t* br_policy;
    double *v_opt, *v_pi;
};

// LDS of an equilibrium block: 8-byte arrays first, then 2-byte (each padded to 16 bytes), then the fixed words: at most
// kTaEqLdsPerTuple * T + kTaEqLdsFixed + 144 bytes, 144.3 KB at T = 4096, whatever N is
inline void ta_eq_layout(TaEqArgs& a) {
    const int T = a.T;
    const int b8 = (8 * T + 15) & ~15, b2 = (2 * T + 15) & ~15;
    int off = 0;
    a.o_va = off; off += b8;
    a.o_vb = off; off += b8;
    a.o_rew = off; off += b8;
    a.o_na = off; off += b2;
    a.o_nb = off; off += b2;
    a.o_sigma = off; off += b2;
    a.o_jn = off; off += b2;
    a.o_mark = off; off += b2;
    a.o_base = off; off += b2;
    a.o_misc = off; off += kTaEqLdsFixed;
    a.lds_bytes = off;
}

int launch_ta_deviation(const TaDevArgs& a, hipStream_t s);
int launch_ta_equilibrium(const TaEqArgs& a, int grid, hipStream_t s);

}  // namespace thrl
