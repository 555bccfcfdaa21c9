// thrl_sampled_response.h -- launch arguments of the best response to sampled play (thrl_sampled_response,
// include/thrl_response.h).  thrl_api_analysis.hip validates; sr_layout() is the one place the LDS layout is written down
// (the API's plan, the header's text and th_rl_amd.sampled_response.working_set follow it); thrl_sampled_response.hip
// holds the kernel.
#pragma once
#include "thrl_sampled.h"

namespace thrl {

constexpr int kSrMaxBlocksPerCu = 8;
constexpr int kSrMaxTeamBytes = 32 * 1024;     // the Q(d, k) staging of a team split, at most

struct SrArgs {
    SpArgs sp;                                 // what sp_stage_game / sp_normaliser read: G, N, T, D, kind, n_actions, tstride,
                                               // eps, eps_g, prob, dpolicy, grp_first, grp_perm, reward, o_row, o_cst, o_prod,
                                               // o_first, o_perm; sp.lds_bytes is the whole block's
    int32_t agents;                            // bit i: agent i is solved
    int32_t max_sweeps;
    int32_t team;                              // threads that share the actions of one price (a power of two; 1: none)
    // byte offsets into the block's LDS (each array starts on a multiple of 16)
    int32_t o_va, o_vb, o_vpi, o_zm, o_si, o_u, o_rt, o_trow, o_sigma, o_modal, o_q;
    double eval_tol;
    double gamma[kSpMaxA];
    const double* sweep_gamma;                 // [N][G] or NULL
    const double* pi;                          // [G][T] or NULL
    int32_t *iters, *sweeps, *n_diff;          // [N][G]
    double *loss_all, *loss_mean, *loss_w, *gain_w, *v_w, *br_prob_w;
    uint16_t* br_policy;                       // [N][G][D] or NULL
    double *v_opt, *v_pi;
};

// The LDS layout of include/thrl_response.h's working set; returns the bytes of a block (also left in a.sp.lds_bytes,
// clamped to INT32_MAX).  team: the largest power of two with team * D <= 256 whose staging of 8 D max_i A_i bytes stays
// within kSrMaxTeamBytes, else 1 (no staging).
inline int64_t sr_layout(SrArgs& a) {
    const int64_t D = a.sp.D;
    int64_t maxA = 1;
    for (int i = 0; i < a.sp.N; i++) maxA = a.sp.n_actions[i] > maxA ? a.sp.n_actions[i] : maxA;
    int team = 1;
    while ((int64_t)team * 2 * D <= kSpBlock && team * 2 <= maxA) team *= 2;
    if (8 * D * maxA > kSrMaxTeamBytes) team = 1;
    a.team = team;
    int64_t off = sr_layout_head(a, D);
    a.sp.o_prod = (int32_t)off; off += 8 * kSpBlock;
    a.o_q = (int32_t)off; off += team > 1 ? r16(8 * D * maxA) : 0;
    a.sp.o_cst = (int32_t)off; off += 256;
    a.sp.lds_bytes = off > INT32_MAX ? INT32_MAX : (int32_t)off;
    return off;
}

#ifndef THRL_SP_HOST_BUILD
int launch_sampled_response(const SrArgs& a, int grid, hipStream_t s);
#endif

}  // namespace thrl
