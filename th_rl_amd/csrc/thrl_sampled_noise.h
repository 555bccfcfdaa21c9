// thrl_sampled_noise.h -- launch arguments of sampled play under demand noise (thrl_sampled_noise_chain, include/thrl.h).
// thrl_api_analysis.hip validates; spn_layout() is the one place the LDS layout is written down (the API's plan, the header's
// text and th_rl_amd.sampled_play.working_set follow it); thrl_sampled_noise.hip holds the kernels.
#pragma once
#include "thrl_sampled.h"

namespace thrl {

constexpr int kSpnTile = 64;                   // nodes of one streamed tile of the networks' node rows
constexpr int kSpnMaxA = 32;                   // actions of a network (thrl_policy.h)
// 16-byte words a thread stages per network and tile: the tile's floats plus up to 3 of alignment lead
constexpr int kSpnChunks = ((kSpnTile * kSpnMaxA + 3 + 3) / 4 + kSpBlock - 1) / kSpBlock;

struct SpnArgs {
    SpArgs sp;                                 // the noise-free half, exactly thrl_sampled_chain's; sp.lds_bytes is the whole block's
    int32_t Jn, W;                             // nodes, band width
    int32_t start_reset;                       // m_0 = the tuple played at a uniform price on [0, a)
    int32_t o_v;                               // double [Jn]: nu, then V = nu / Zn tile by tile
    int32_t o_nrow[kSpMaxA];                   // QTable agent i's node entries: uint16 [Jn]
    int32_t o_tile[kSpMaxA][2];                // network i's two tile buffers: float [kSpnTile * A_i + 3], in 16-byte words
    double noise_prob;
    const double* noise_prob_g;                // [G] or NULL
    const float* nprob[kSpMaxA];               // [G][Jn][A_i] (networks)
    const uint16_t* npolicy;                   // [G][N][Jn]
    const int32_t* band_lo;                    // [T]
    const double* band;                        // [T][W]
    const double* noise_price;                 // [T]
    const double* noise_reward;                // [N][T]
    const double* node_w;                      // [Jn] (start_reset)
    double* max_jump;                          // [G] or NULL
};

// the LDS layout of include/thrl.h's working set: sp_layout's arrays, then V, the QTable agents' node entries and the
// networks' double-buffered tiles; returns the bytes of a block (also left in a.sp.lds_bytes)
inline int64_t spn_layout(SpnArgs& a) {
    int64_t off = sp_layout(a.sp);
    a.o_v = (int32_t)off; off += r16(8 * (int64_t)a.Jn);
    for (int i = 0; i < a.sp.N; i++) {
        a.o_nrow[i] = a.o_tile[i][0] = a.o_tile[i][1] = 0;
        if (a.sp.kind[i] == 0) {
            a.o_nrow[i] = (int32_t)off; off += r16(2 * (int64_t)a.Jn);
        } else {
            const int64_t b = r16(4 * ((int64_t)kSpnTile * a.sp.n_actions[i] + 3));
            a.o_tile[i][0] = (int32_t)off; off += b;
            a.o_tile[i][1] = (int32_t)off; off += b;
        }
    }
    a.sp.lds_bytes = off > INT32_MAX ? INT32_MAX : (int32_t)off;
    return off;
}

#ifndef THRL_SP_HOST_BUILD
int launch_sampled_noise_chain(const SpnArgs& a, int grid, hipStream_t s);
#endif

}  // namespace thrl
