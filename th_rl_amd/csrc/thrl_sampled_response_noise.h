// thrl_sampled_response_noise.h -- launch arguments of the best response to sampled play under demand noise
// (thrl_sampled_response_noise, include/thrl_response_noise.h).  thrl_api_analysis.hip validates; srn_layout() is the one
// place the LDS layout is written down (the API's plan, the header's text and
// th_rl_amd.sampled_response.working_set_noise follow it); thrl_sampled_response_noise.hip holds the kernel.
#pragma once
#include "thrl_sampled.h"

namespace thrl {

constexpr int kSrnMaxBlocksPerCu = 4;            // four waves per SIMD by registers (profiles/sampled_response_noise_resource_usage.txt)

struct SrnArgs {
    SpArgs sp;                                 // what sp_stage_game reads: G, N, T, D, kind, n_actions, tstride, eps, eps_g,
                                               // prob, dpolicy, grp_first, grp_perm, reward, o_row, o_cst, o_prod, o_first,
                                               // o_perm; sp.lds_bytes is the whole block's
    int32_t Jn, W;                             // nodes, band width; the states are the D prices, then the Jn nodes
    int32_t agents;                            // bit i: agent i is solved
    int32_t max_sweeps;
    // byte offsets into the block's LDS (each array starts on a multiple of 16); the arrays over the states are [D + Jn]
    int32_t o_va, o_vb, o_vpi, o_zm, o_si, o_u, o_rt, o_trow, o_sigma, o_modal;
    int32_t o_nrow[kSpMaxA];                   // QTable agent i's node entries: uint16 [Jn]
    const double* sweep_gamma;                 // [N][G] or NULL
    const double* noise_prob_g;                // [G] or NULL
    const double* pi;                          // [G][T] or NULL
    const float* nprob[kSpMaxA];               // [G][Jn][A_i] (networks): read from global memory every sweep
    const uint16_t* npolicy;                   // [G][N][Jn]
    const int32_t* band_lo;                    // [T]
    const double* band;                        // [T][W]
    const double* noise_reward;                // [N][T]
    double eval_tol;
    double noise_prob;
    double gamma[kSpMaxA];
    int32_t *iters, *sweeps, *n_diff_prices, *n_diff_nodes;            // [N][G]
    double *loss_all, *loss_prices_mean, *loss_nodes_mean, *loss_w, *gain_w, *v_w, *br_prob_w;
    uint16_t* br_policy;                       // [N][G][D + Jn] or NULL
    double *v_opt, *v_pi;
};

// The LDS layout of include/thrl_response_noise.h's working set, S = D + Jn:
//   5 r16(8 S) + 2 r16(8 T) + sum_i (QTable i: r16(2 D); network i: r16(4 D A_i)) + r16(2 (D + 1)) + 2 r16(2 T)
//   + 2 r16(2 S) + sum over the QTable agents of r16(2 Jn) + 2,048 + 256
// returns the bytes of a block (also left in a.sp.lds_bytes, clamped to INT32_MAX).  The networks' node rows are not part
// of it: they stay in global memory.
inline int64_t srn_layout(SrnArgs& a) {
    const int64_t Jn = a.Jn;
    int64_t off = sr_layout_head(a, a.sp.D + Jn);
    for (int i = 0; i < a.sp.N; i++) {
        a.o_nrow[i] = 0;
        if (a.sp.kind[i] == 0) { a.o_nrow[i] = (int32_t)off; off += r16(2 * Jn); }
    }
    a.sp.o_prod = (int32_t)off; off += 8 * kSpBlock;
    a.sp.o_cst = (int32_t)off; off += 256;
    a.sp.lds_bytes = off > INT32_MAX ? INT32_MAX : (int32_t)off;
    return off;
}

#ifndef THRL_SP_HOST_BUILD
int launch_sampled_response_noise(const SrnArgs& a, int grid, hipStream_t s);
#endif

}  // namespace thrl
