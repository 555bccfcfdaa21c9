// thrl_equilibrium_noise.h -- launch arguments of the equilibrium check under demand noise (thrl_equilibrium_noise,
// include/thrl.h).  thrl_api_analysis.hip validates and takes the per-config plan of thrl_equilibrium (the rewards per
// tuple) from its cache, eqn_layout() lays out LDS; thrl_equilibrium_noise.hip holds the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thrl_device.h"

namespace thrl {

constexpr int kEqnLdsBudget = 64 * 1024;       // per one-wave block
constexpr int kEqnMaxBlocksPerCu = 32;
constexpr int kEqnSums = 4;                    // ordered sums: loss, w * loss, w * [differs], w * V_pi

struct EqnArgs {
    int32_t G, N, T, P, J, W;
    int32_t agents;
    int32_t max_sweeps;
    int32_t zt_lds;                            // z per tuple has its 8 T bytes of LDS
    int32_t lds_bytes;
    // byte offsets into the block's LDS
    int32_t o_va, o_vb, o_vpi, o_rs, o_prod, o_zt, o_blo, o_tcur, o_sigma, o_base, o_pol, o_tup, o_det;
    double noise_prob, eval_tol;
    AgentParams ag[THRL_MAXA];
    int32_t tstride[THRL_MAXA];                // tuple index = sum_i a_i * tstride[i] (agent 0 slowest)
    int32_t row_off[THRL_MAXA];                // first policy entry of agent i in a game's P entries
    const uint16_t* policy;                    // [G][P]
    const double* noise_prob_g;                // [G] or NULL
    const double* sweep_gamma;                 // [N][G] or NULL
    const double* rew;                         // plan, device: [N][T] reward of agent i at tuple t
    const int32_t* cell_rows;                  // [N][J]
    const int32_t* det_cell;                   // [T]
    const int32_t* band_lo;                    // [T]
    const double* band;                        // [T][W]
    const double* noise_reward;                // [N][T]
    const double* weights;                     // [G][J] or NULL
    int32_t *iters, *sweeps, *n_diff_all;      // [N][G]
    double *loss_all, *loss_all_mean, *loss_w, *diff_w, *v_w;
    uint16_t* br_policy;                       // [N][G][J] or NULL
    double *v_opt, *v_pi;
};

// LDS of a block, from J and T: 8-byte arrays first, then 4-byte, then 2-byte.  Returns the bytes a game needs (50 J +
// 2064: refused over the budget); z per tuple is staged where its 8 T bytes fit beside them.
inline int64_t eqn_layout(EqnArgs& a) {
    const int64_t J = a.J;
    const int64_t need = 50 * J + 8 * 64 * kEqnSums + 16;
    a.zt_lds = need + 8 * (int64_t)a.T <= kEqnLdsBudget;
    if (need > kEqnLdsBudget) return need;
    int off = 0;
    a.o_va = off; off += 8 * a.J;
    a.o_vb = off; off += 8 * a.J;
    a.o_vpi = off; off += 8 * a.J;
    a.o_rs = off; off += 8 * a.J;
    a.o_prod = off; off += 8 * 64 * kEqnSums;
    a.o_zt = off; off += a.zt_lds ? 8 * a.T : 0;
    a.o_blo = off; off += 4 * a.J;
    a.o_tcur = off; off += 4 * a.J;
    a.o_sigma = off; off += 2 * a.J;
    a.o_base = off; off += 2 * a.J;
    a.o_pol = off; off += 2 * a.J;
    a.o_tup = off; off += 2 * a.J;
    a.o_det = off; off += 2 * a.J;
    a.lds_bytes = (off + 15) & ~15;
    return need;
}

int launch_equilibrium_noise(const EqnArgs& a, int grid, hipStream_t s);

}  // namespace thrl
