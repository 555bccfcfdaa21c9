// thrl_tuple_attractors.h -- launch arguments of the attractor analysis in tuple form (thrl_tuple_attractors,
// include/thrl.h).  thrl_api_analysis.hip validates, tat_layout() lays out LDS; thrl_tuple_attractors.hip holds the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thrl_device.h"

namespace thrl {

constexpr int kTatBlock = 256;                 // threads of the block that analyses one game
constexpr int kTatMaxBlocksPerCu = 7;          // the kernel's 71 VGPRs leave 7 waves per SIMD: seven 4-wave blocks per CU
// bytes of LDS per tuple: basin and cycle-length counters (4 + 4), the map F, two map buffers and two minimum / step
// buffers of the doubling passes, rep, the on-cycle flag and the slot of the tuple's rep (2 each)
constexpr int kTatLdsPerTuple = 26;

struct TatArgs {
    int32_t G, N, T, L;                        // L = ceil(log2 T): doubling rounds of either pass
    int32_t lds_bytes;
    // byte offsets into the block's LDS
    int32_t o_cw, o_cprod, o_cmean, o_basin, o_lamc, o_sel, o_red, o_f, o_pa, o_pb, o_ma, o_mb, o_rep, o_on, o_slot,
        o_cslot;
    int32_t n_actions[THRL_MAXA];
    int32_t tstride[THRL_MAXA];                // prod_{j > i} n_actions[j]: agent 0 slowest
    const int32_t* start;                      // [G]
    const uint16_t* policy;                    // [G][N][T]
    const double* reward;                      // [N][T]
    const double* scaled;                      // [N][T]
    const double* start_w;                     // [T] or null
    int32_t *n_attr, *mu_max, *n_cycle_states, *rep, *lam, *basin, *rep_x0, *mu_x0, *slot_x0;
    double *cycle_reward, *cycle_action, *start_mass, *start_mass_other, *start_reward;
    uint16_t *tuple_rep, *tuple_mu;            // [G][T] or null
};

// LDS of a block: 8-byte arrays first, then 4-byte, then 2-byte (each padded to 16 bytes): kTatLdsPerTuple * T plus
// the staging of a chunk of start weights, (8 * (1 + N) + 2) * kTatBlock bytes, and under 1 KB of fixed words:
// 102.7 KB at T = 4096 with two agents, 115.1 KB with eight
inline void tat_layout(TatArgs& a) {
    const int T = a.T, N = a.N;
    const int b4 = (4 * T + 15) & ~15, b2 = (2 * T + 15) & ~15;
    int off = 0;
    a.o_cw = off; off += 8 * kTatBlock;
    a.o_cprod = off; off += 8 * kTatBlock * N;
    a.o_cmean = off; off += 8 * THRL_ATTR_KEEP * N;
    a.o_basin = off; off += b4;
    a.o_lamc = off; off += b4;
    a.o_sel = off; off += 4 * THRL_ATTR_KEEP;
    a.o_red = off; off += 4 * 20;
    off = (off + 15) & ~15;
    a.o_f = off; off += b2;
    a.o_pa = off; off += b2;
    a.o_pb = off; off += b2;
    a.o_ma = off; off += b2;
    a.o_mb = off; off += b2;
    a.o_rep = off; off += b2;
    a.o_on = off; off += b2;
    a.o_slot = off; off += b2;
    a.o_cslot = off; off += 2 * kTatBlock;
    a.lds_bytes = off;
}

int launch_tuple_attractors(const TatArgs& a, int grid, hipStream_t s);

}  // namespace thrl
