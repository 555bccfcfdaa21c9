// thrl_sampled_deviation_noise.h -- launch arguments of the deviation test of sampled play under demand noise
// (thrl_sampled_deviation_noise, include/thrl_sampled_deviation_noise.h).  thrl_api_analysis.hip validates; sdn_layout()
// is the one place the LDS layout is written down (the API's plan, the header's text and
// th_rl_amd.sampled_deviation.working_set_noise follow it); thrl_sampled_deviation_noise.hip holds the kernel.
#pragma once
#include "thrl_sampled_deviation.h"
#include "thrl_sampled_noise.h"

namespace thrl {

constexpr int kSdnMaxBlocksPerCu = 8;

struct SdnArgs {
    SpnArgs n;                                 // the chain under noise, exactly thrl_sampled_noise_chain's: n.sp is the SpArgs
                                               // every shared function reads, n.sp.lds_bytes the whole block's
    SdArgs sd;                                 // the deviation, its bookkeeping and the outputs, exactly
                                               // thrl_sampled_deviation's; sd.sp is not filled and nothing reads it.  o_ad is
                                               // ad_g over the S = D + Jn states, dev_policy is [G][S]
};

// The LDS layout of include/thrl_sampled_deviation_noise.h's working set: spn_layout's arrays, then ad_g over the states
// (2 S), the deviation step's Z (8 D) and one more staging row of 64 terms (512) for the distance.  Returns the bytes of a
// block (also left in a.n.sp.lds_bytes, clamped to INT32_MAX); the caller has filled a.n's head.
inline int64_t sdn_layout(SdnArgs& a) {
    int64_t off = spn_layout(a.n);
    a.sd.o_ad = (int32_t)off; off += r16(2 * ((int64_t)a.n.sp.D + a.n.Jn));
    a.sd.o_zd = (int32_t)off; off += r16(8 * (int64_t)a.n.sp.D);
    a.sd.o_dist = (int32_t)off; off += 512;
    a.n.sp.lds_bytes = off > INT32_MAX ? INT32_MAX : (int32_t)off;
    return off;
}

#ifndef THRL_SP_HOST_BUILD
int launch_sampled_deviation_noise(const SdnArgs& a, int grid, hipStream_t s);
#endif

}  // namespace thrl
