// thrl_tuple_stationary.h -- launch arguments of the stationary analysis in tuple form (thrl_tuple_stationary,
// include/thrl.h).  thrl_api_analysis.hip validates, ts_layout() lays out LDS; thrl_tuple_stationary.hip holds the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thrl_device.h"

namespace thrl {

constexpr int kTsBlock = 256;                  // threads of a game's block
constexpr int kTsMaxBlocksPerCu = 8;

struct TsArgs {
    int32_t G, N, T, J, W;
    int32_t max_iters;
    int32_t start_tuple;                       // m_0 = the unit mass on start[g] (else the reset distribution)
    int32_t neural_mask;                       // bit i: agent i is a network (n_switch / unresolved)
    int32_t lds_bytes;
    // byte offsets into the block's LDS; nu follows mb directly (the sort scratch of the groupings spans both)
    int32_t o_ma, o_mb, o_nu, o_prod, o_permk, o_startk, o_permt, o_startt;
    double noise_prob, tol;
    int32_t n_actions[THRL_MAXA];
    int32_t tstride[THRL_MAXA];                // prod_{j > i} n_actions[j]: agent 0 slowest
    const double* noise_prob_g;                // [G] or NULL
    const int32_t* start;                      // [G] (start_tuple)
    const uint16_t* tuple_policy;              // [G][N][T]
    const uint16_t* cell_policy;               // [G][N][J]
    const double* cell_w;                      // [J]
    const double* reward;                      // [N][T]
    const double* scaled;                      // [N][T]
    const double* price;                       // [T]
    const int32_t* band_lo;                    // [T]
    const double* band;                        // [T][W]
    const double* noise_reward;                // [N][T]
    const double* noise_price;                 // [T]
    int32_t* iters;
    double *change, *mass, *stat_reward, *stat_action, *stat_price, *pi;
    int32_t* n_switch;
    double* unresolved;
};

// LDS of a block (the working set of include/thrl.h): 8-byte arrays first, nu directly behind the second iterate,
// then the 2-byte arrays of the two groupings
inline void ts_layout(TsArgs& a) {
    const int T = a.T, J = a.J, N = a.N;
    int off = 0;
    a.o_ma = off; off += 8 * T;
    a.o_mb = off; off += 8 * T;
    a.o_nu = off; off += 8 * J;
    a.o_prod = off; off += 8 * 64 * (2 * N + 2);
    a.o_permk = off; off += 2 * J;
    a.o_startk = off; off += 2 * (T + 1);
    a.o_permt = off; off += 2 * T;
    a.o_startt = off; off += 2 * (T + 1);
    a.lds_bytes = (off + 15) & ~15;
}

int launch_tuple_stationary(const TsArgs& a, int grid, hipStream_t s);

}  // namespace thrl
