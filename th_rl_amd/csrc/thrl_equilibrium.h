// thrl_equilibrium.h -- launch arguments of the equilibrium-check kernel (thrl_equilibrium, include/thrl.h).
// thrl_api.hip validates, builds the per-config plan (tuple LUTs, state rows) and lays out LDS; thrl_equilibrium.hip
// holds the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thrl_device.h"

namespace thrl {

constexpr int kEqLdsBudget = 64 * 1024;        // per one-wave block; the reward LUT moves to global memory if it does not fit
constexpr int kEqMaxBlocksPerCu = 16;

struct EqArgs {
    int32_t G, N, S, T;
    int32_t agents;                            // bit i: solve agent i
    int32_t small;                             // S <= 64: V and n of the evaluation live in registers
    int32_t lut_lds;                           // the reward LUT is staged in LDS
    int32_t lds_bytes;
    // byte offsets into the block's LDS
    int32_t o_va, o_vb, o_vpi, o_rew, o_base, o_first, o_x0row, o_sid, o_pol, o_sigma, o_jn, o_na, o_nb;
    int64_t stride;
    AgentParams ag[THRL_MAXA];
    int32_t tstride[THRL_MAXA];                // tuple index = sum_i a_i * tstride[i] (agent 0 slowest)
    const void* q;
    const double* state0;
    const double* sweep_gamma;
    const double* rew;                         // plan, device: [N][T] reward of agent i at tuple t
    const int32_t* srow;                       //               [N][S] row of agent i in state s
    const uint16_t* sid;                       //               [T]    state of tuple t
    int32_t *mu, *lam, *iters, *n_diff_all, *n_diff_on;
    double *loss_all, *loss_on, *loss_all_mean, *loss_on_mean, *v_on;
    uint16_t* br_policy;
    double *v_opt, *v_pi;
};

int launch_equilibrium(const EqArgs& a, int q_dtype, int grid, hipStream_t s);

}  // namespace thrl
