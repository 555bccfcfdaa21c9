// thrl_deviation_noise.h -- launch arguments of the deviation test under demand noise (thrl_deviation_noise,
// include/thrl.h).  thrl_api_analysis.hip validates and takes the per-config plan of thrl_equilibrium (the rewards per
// tuple) from its cache, devn_layout() lays out LDS; thrl_deviation_noise.hip holds the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thrl_device.h"

namespace thrl {

constexpr int kDevnLdsBudget = 64 * 1024;      // per one-wave block
constexpr int kDevnMaxBlocksPerCu = 32;

struct DevnArgs {
    int32_t G, N, T, P, J, W;
    int32_t d, L, K, dev_action;               // deviator, dev_len, n_steps, fixed action or -1
    int32_t row_begin, row_count;
    int32_t lds_bytes;
    // byte offsets into the block's LDS
    int32_t o_mua, o_mub, o_prod, o_tup, o_tupd;
    double noise_prob, ret_tol, gamma_d;
    AgentParams ag[THRL_MAXA];
    int32_t tstride[THRL_MAXA];                // tuple index = sum_i a_i * tstride[i] (agent 0 slowest)
    int32_t row_off[THRL_MAXA];                // first policy entry of agent i in a game's P entries
    const uint16_t* policy;                    // [G][P]
    const double* noise_prob_g;                // [G] or NULL
    const double* sweep_gamma;                 // [N][G] or NULL
    const double* weights;                     // [G][J]: m_0
    const double* rew;                         // plan, device: [N][T] reward of agent i at tuple t
    const int32_t* cell_rows;                  // [N][J]
    const int32_t* det_cell;                   // [T]
    const int32_t* band_lo;                    // [T]
    const double* band;                        // [T][W]
    const double* noise_reward;                // [N][T]
    double *base_reward, *base_action;         // [N][G]
    double *dev_share, *gain, *gain_dev, *low, *dist, *mass;   // [G]
    int32_t *low_step, *ret_step;              // [G]
    double *reward_rows, *action_rows;         // [row_count][N][G] or NULL
    double* dist_rows;                         // [row_count][G] or NULL
};

// LDS of a block, from N and J: the two iterates, the staging of the ordered sums [2N + 2][64], then the tuples t(k) and
// t'(k).  Returns the bytes a game needs (20 J + 512 (2N + 2) + 16: refused over the budget).  The per-cell det / band
// places are never staged: the step reads them through the source's tuple.
inline int64_t devn_layout(DevnArgs& a) {
    const int N = a.N;
    const int64_t J = a.J;
    const int64_t need = 20 * J + 8 * 64 * (int64_t)(2 * N + 2) + 16;
    if (need > kDevnLdsBudget) return need;
    int off = 0;
    a.o_mua = off; off += 8 * a.J;
    a.o_mub = off; off += 8 * a.J;
    a.o_prod = off; off += 8 * 64 * (2 * N + 2);
    a.o_tup = off; off += 2 * a.J;
    a.o_tupd = off; off += 2 * a.J;
    a.lds_bytes = (off + 15) & ~15;
    return need;
}

int launch_deviation_noise(const DevnArgs& a, int grid, hipStream_t s);

}  // namespace thrl
