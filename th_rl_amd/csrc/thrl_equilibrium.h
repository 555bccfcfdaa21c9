// thrl_equilibrium.h -- launch arguments of the equilibrium-check kernel (thrl_equilibrium, include/thrl.h).
// thrl_api_analysis.hip validates and builds the per-config plan (tuple LUTs, state rows), eq_layout() lays out LDS;
// thrl_equilibrium.hip holds the kernel.
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

// LDS of a block: 8-byte arrays first, then 4-byte, then 2-byte (lds_bytes over the budget is refused by the caller)
inline void eq_layout(EqArgs& a) {
    const int S = a.S, T = a.T, N = a.N;
    const int64_t fixed = 3 * 8 * (int64_t)S + 4 * (int64_t)S + 4 * THRL_MAXA
                          + 2 * ((int64_t)T + (int64_t)N * S + THRL_MAXA + 5 * (int64_t)S) + 64;
    a.lut_lds = fixed + 8 * (int64_t)N * T <= kEqLdsBudget;
    int off = 0;
    a.o_va = off; off += 8 * S;
    a.o_vb = off; off += 8 * S;
    a.o_vpi = off; off += 8 * S;
    a.o_rew = off; off += a.lut_lds ? 8 * N * T : 0;
    a.o_base = off; off += 4 * S;
    a.o_x0row = off; off += 4 * THRL_MAXA;
    a.o_sid = off; off += 2 * T;
    a.o_first = off; off += 2 * S;
    a.o_pol = off; off += 2 * (N * S + THRL_MAXA);
    a.o_sigma = off; off += 2 * S;
    a.o_jn = off; off += 2 * S;
    a.o_na = off; off += 2 * S;
    a.o_nb = off; off += 2 * S;
    a.lds_bytes = (off + 15) & ~15;
}

int launch_equilibrium(const EqArgs& a, int q_dtype, int grid, hipStream_t s);

}  // namespace thrl
