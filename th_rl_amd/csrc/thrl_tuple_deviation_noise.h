// thrl_tuple_deviation_noise.h -- launch arguments of the deviation test under demand noise in tuple form
// (thrl_tuple_deviation_noise, include/thrl.h).  thrl_api_analysis.hip validates, tdn_layout() lays out LDS;
// thrl_tuple_deviation_noise.hip holds the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thrl_device.h"

namespace thrl {

constexpr int kTdnBlock = 256;                 // threads of a game's block
constexpr int kTdnMaxBlocksPerCu = 8;

struct TdnArgs {
    int32_t G, N, T, J, W;
    int32_t d, L, K, dev_action;               // deviator, dev_len, n_steps, fixed action or -1
    int32_t row_begin, row_count;
    int32_t lds_bytes;
    // byte offsets into the block's LDS; nu follows mb directly (the sort scratch of the groupings spans both)
    int32_t o_ma, o_mb, o_nu, o_prod, o_permk, o_startk, o_permd, o_startd, o_permt, o_startt, o_dv;
    double noise_prob, ret_tol, gamma_d;
    int32_t n_actions[THRL_MAXA];
    int32_t tstride[THRL_MAXA];                // prod_{j > i} n_actions[j]: agent 0 slowest
    const double* noise_prob_g;                // [G] or NULL
    const double* sweep_gamma;                 // [N][G] or NULL
    const uint16_t* tuple_policy;              // [G][N][T]
    const uint16_t* cell_policy;               // [G][N][J]
    const double* reward;                      // [N][T]
    const double* scaled;                      // [N][T]
    const int32_t* band_lo;                    // [T]
    const double* band;                        // [T][W]
    const double* noise_reward;                // [N][T]
    const double* weights;                     // [G][T]: m_0
    double *base_reward, *base_action;         // [N][G]
    double *dev_share, *gain, *gain_dev, *low, *dist, *mass;   // [G]
    int32_t *low_step, *ret_step;              // [G]
    double *reward_rows, *action_rows;         // [row_count][N][G] or NULL
    double* dist_rows;                         // [row_count][G] or NULL
};

// LDS of a block (the working set of include/thrl.h), from N, T and J: 8-byte arrays first, nu directly behind the second
// iterate, the staging of the ordered sums [2N + 2][64], then the 2-byte arrays: the grouping of the cells by tau_g, of
// the tuples by F_g o Dv_g and by F_g, and Dv_g.  Returns the bytes a game needs: 28 T + 10 J + 512 (2N + 2) + 6, rounded
// up to 16.
inline int64_t tdn_layout(TdnArgs& a) {
    const int64_t T = a.T, J = a.J, N = a.N;
    int64_t off = 0;
    a.o_ma = (int32_t)off; off += 8 * T;
    a.o_mb = (int32_t)off; off += 8 * T;
    a.o_nu = (int32_t)off; off += 8 * J;
    a.o_prod = (int32_t)off; off += 8 * 64 * (2 * N + 2);
    a.o_permk = (int32_t)off; off += 2 * J;
    a.o_startk = (int32_t)off; off += 2 * (T + 1);
    a.o_permd = (int32_t)off; off += 2 * T;
    a.o_startd = (int32_t)off; off += 2 * (T + 1);
    a.o_permt = (int32_t)off; off += 2 * T;
    a.o_startt = (int32_t)off; off += 2 * (T + 1);
    a.o_dv = (int32_t)off; off += 2 * T;
    const int64_t need = (off + 15) & ~(int64_t)15;
    a.lds_bytes = (int32_t)need;
    return need;
}

int launch_tuple_deviation_noise(const TdnArgs& a, int grid, hipStream_t s);

}  // namespace thrl
