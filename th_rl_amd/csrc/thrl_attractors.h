// thrl_attractors.h -- launch arguments of the attractor-analysis kernel (thrl_attractors, include/thrl.h).
// thrl_api_analysis.hip validates and takes the per-config plan of thrl_equilibrium (tuple LUTs, state rows) from its
// cache, attr_layout() lays out LDS; thrl_attractors.hip holds the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thrl_device.h"

namespace thrl {

constexpr int kAttrLdsBudget = 64 * 1024;      // per one-wave block; the reward LUT moves to global memory if it does not fit
constexpr int kAttrMaxBlocksPerCu = 16;

struct AttrArgs {
    int32_t G, N, S, T, P, J;
    int32_t L;                                 // doubling rounds: the smallest L with 2^L >= S
    int32_t lut_lds;                           // the reward LUT is staged in LDS
    int32_t lds_bytes;
    // byte offsets into the block's LDS
    int32_t o_rew, o_cw, o_cprod, o_basin, o_lamc, o_x0row, o_sel, o_cslot, o_sid, o_pol, o_lev, o_ma, o_mb, o_rep, o_mu,
        o_on, o_tup, o_slot;
    AgentParams ag[THRL_MAXA];
    int32_t tstride[THRL_MAXA];                // tuple index = sum_i a_i * tstride[i] (agent 0 slowest)
    int32_t row_off[THRL_MAXA];                // first policy entry of agent i in a game's P entries
    const uint16_t* policy;                    // [G][P]
    const double* state0;
    const double* rew;                         // plan, device: [N][T] reward of agent i at tuple t
    const int32_t* srow;                       //               [N][S] row of agent i in state s
    const uint16_t* sid;                       //               [T]    state of tuple t
    const int32_t* start_rows;                 // [N][J]
    const double* start_w;                     // [J]
    int32_t *n_attr, *mu_max, *n_cycle_states;
    int32_t *rep, *lam, *basin;
    double *cycle_reward, *cycle_action;
    int32_t *rep_x0, *mu_x0, *slot_x0;
    double *reset_mass, *reset_mass_other, *reset_reward;
    uint16_t *state_rep, *state_mu;
};

// LDS of a block: 8-byte arrays first, then 4-byte, then 2-byte.  Returns the bytes without the reward LUT (refused over the budget).
inline int64_t attr_layout(AttrArgs& a) {
    const int S = a.S, T = a.T, N = a.N;
    const int64_t fixed = 8 * 64 * (int64_t)(1 + N) + 4 * (2 * (int64_t)S + THRL_MAXA + THRL_ATTR_KEEP + 64)
                          + 2 * ((int64_t)T + (int64_t)N * S + THRL_MAXA + (int64_t)(a.L + 1) * S + 7 * (int64_t)S) + 64;
    a.lut_lds = fixed + 8 * (int64_t)N * T <= kAttrLdsBudget;
    int off = 0;
    a.o_rew = off; off += a.lut_lds ? 8 * N * T : 0;
    a.o_cw = off; off += 8 * 64;
    a.o_cprod = off; off += 8 * 64 * N;
    a.o_basin = off; off += 4 * S;
    a.o_lamc = off; off += 4 * S;
    a.o_x0row = off; off += 4 * THRL_MAXA;
    a.o_sel = off; off += 4 * THRL_ATTR_KEEP;
    a.o_cslot = off; off += 4 * 64;
    a.o_sid = off; off += 2 * T;
    a.o_pol = off; off += 2 * (N * S + THRL_MAXA);
    a.o_lev = off; off += 2 * (a.L + 1) * S;
    a.o_ma = off; off += 2 * S;
    a.o_mb = off; off += 2 * S;
    a.o_rep = off; off += 2 * S;
    a.o_mu = off; off += 2 * S;
    a.o_on = off; off += 2 * S;
    a.o_tup = off; off += 2 * S;
    a.o_slot = off; off += 2 * S;
    a.lds_bytes = (off + 15) & ~15;
    return fixed;
}

int launch_attractors(const AttrArgs& a, int grid, hipStream_t s);

}  // namespace thrl
