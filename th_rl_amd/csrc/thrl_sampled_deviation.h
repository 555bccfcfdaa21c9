// thrl_sampled_deviation.h -- launch arguments of the deviation test of sampled play (thrl_sampled_deviation,
// include/thrl_sampled_deviation.h).  thrl_api_analysis.hip validates; sd_layout() is the one place the LDS layout is
// written down (the API's plan, the header's text and th_rl_amd.sampled_deviation.working_set follow it);
// thrl_sampled_deviation.hip holds the kernel.
#pragma once
#include "thrl_sampled.h"

namespace thrl {

constexpr int kSdMaxBlocksPerCu = 8;

struct SdArgs {
    SpArgs sp;                                 // what sp_stage_game, sp_normaliser, sp_weights and sp_price_sum read, and
                                               // the LDS offsets of sp_layout; sp.lds_bytes is the whole block's
    // The fields below come in runs of 16 bytes with a word between them that nothing reads.  The compiler merges the
    // scalar loads of neighbouring fields; of this struct it spilled two 256-bit tuples whole and kept their stack slots
    // (68 bytes of scratch reserved, never accessed).  A gap ends a merge, so no load here is wider than 128 bits.
    int32_t d, L, K;                           // deviator, dev_len, n_steps
    int32_t dev_action;                        // a fixed action, or -1
    int64_t gap0;
    const double* sweep_gamma;                 // [N][G] or NULL
    const uint16_t* dev_policy;                // [G][D] (use_policy)
    int64_t gap1;
    int32_t use_policy;                        // THRL_SD_POLICY: ad_g = dev_policy
    int32_t row_begin, row_count;
    int32_t o_ad;                              // byte offsets into the block's LDS behind sp_layout's arrays: o_ad, o_zd, o_dist
    int64_t gap2;
    int32_t o_zd, o_dist;
    const double* weights;                     // [G][T]: x_0
    int64_t gap3;
    double gamma, ret_tol;
    int64_t gap4;
    double *base_reward, *base_action;         // [N][G]
    int64_t gap5;
    double *base_price, *dev_share;            // [G], as are gain .. mass
    int64_t gap6;
    double *gain, *gain_dev;
    int64_t gap7;
    double *low, *dist;
    int64_t gap8;
    double* mass;
    int32_t* low_step;                         // [G], as is ret_step
    int64_t gap9;
    int32_t* ret_step;
    double* reward_rows;                       // [row_count][N][G] or NULL, as is action_rows
    int64_t gap10;
    double* action_rows;
    double* price_rows;                        // [row_count][G] or NULL, as is dist_rows
    int64_t gap11;
    double* dist_rows;
};

// The LDS layout of include/thrl_sampled_deviation.h's working set: sp_layout's arrays, then ad_g (2 D), the deviation
// step's Z (8 D) and one more staging row of 64 terms (512) for the distance, the sum a period takes beyond the 2 N + 2 of
// sampled play.  Returns the bytes of a block (also left in a.sp.lds_bytes, clamped to INT32_MAX); the caller has filled
// a.sp's head.
inline int64_t sd_layout(SdArgs& a) {
    int64_t off = sp_layout(a.sp);
    a.o_ad = (int32_t)off; off += r16(2 * (int64_t)a.sp.D);
    a.o_zd = (int32_t)off; off += r16(8 * (int64_t)a.sp.D);
    a.o_dist = (int32_t)off; off += 512;
    a.sp.lds_bytes = off > INT32_MAX ? INT32_MAX : (int32_t)off;
    return off;
}

#ifndef THRL_SP_HOST_BUILD
int launch_sampled_deviation(const SdArgs& a, int grid, hipStream_t s);
#endif

}  // namespace thrl
