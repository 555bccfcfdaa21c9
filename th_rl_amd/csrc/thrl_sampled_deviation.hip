// thrl_sampled_deviation.hip -- the deviation test of SAMPLED play (thrl_sampled_deviation,
// include/thrl_sampled_deviation.h): the expected impulse response of the agents' stochastic policies to a forced
// deviation of one of them, by propagating a distribution over the tuple played through thrl_sampled_chain's chain -- L
// steps with the deviator's row replaced by a deterministic strategy ad_g of the price, then K - L plain steps -- and what
// every period's distribution earns.  One kernel.
//
// k_sd_chain has k_sp_chain's shape: a 256-thread block per game, looping over games, everything in LDS.  Per game the
//   block stages the rows at the distinct prices exactly as k_sp_chain does (sp_stage_game, sp_normaliser), then once:
//   ad_g(d) (uint16 [D]; for a best response the first maximum over k of q(d, k), thrl_response_dev.h's sr_q with U =
//   reward_d staged in the second iterate, which is dead until the first step: a thread per price, k ascending) and the
//   deviation step's Z(d), the product with S_d = 1.0; the terms of dev_share parked over U once it is read.  A step is
//   k_sp_chain's without the lazy half: sp_weights with the step's Z, then a thread per output tuple walking the prices
//   in ascending order (sp_price_sum).  For the deviation step the deviator's staged row is written over: a QTable
//   deviator's greedy row by ad_g with hi = 1.0 and lo = 0.0 in its constants, a network's probabilities by the float32
//   rows that are 1.0 at ad_g(d) and 0.0 elsewhere (exact when widened), so sp_price_sum evaluates the step as it stands;
//   after L periods the game's rows and constants are staged again.  The ordered sums of a period follow k_sp_chain's
//   outputs: chunks of 64 tuples, one lane per tuple for the products, then one lane per sum reading them back in
//   ascending t (chain_read_back), keyed as chain_store keys them -- 0 the mass, 1 .. N the rewards, N + 1 .. 2 N the
//   actions, 2 N + 1 the price -- and lane 2 N + 2 the distance from its own staging row.  The lane of a sum keeps what is
//   derived from it in registers over the periods, as k_tdn_chain does: lane 1 + d the gain and the low, lane 2 N + 2 the
//   distance and ret_step.  x_0 is re-read from global memory (coalesced) for the distance.  No atomic is involved.
//   What this file keeps is the order of a game's passes and the step.  Everything else -- the staging of the grouping,
//   the row sum, the unsolved outputs, ad_g and Z at the prices, dev_share's terms, a period's sums, the baseline's stores,
//   the replaced rows and the lanes' bookkeeping over the periods -- sits in thrl_sampled_deviation_dev.h, one copy that
//   k_sdn_chain calls too.
//   Nothing in the body is wave-specific: with THRL_SP_HOST_BUILD the same source runs as 256 host threads with barriers.
#include "thrl_response_dev.h"
#include "thrl_sampled_deviation.h"
#include "thrl_sampled_deviation_dev.h"

namespace thrl {

namespace {

template <int MAXN>
__device__ __forceinline__ void sd_block(const SdArgs& a, unsigned char* s_mem, int tid, int bid, int nblk) {
    const SpArgs& sp = a.sp;
    const int G = sp.G, T = sp.T, D = sp.D, K = a.K, L = a.L, dv = a.d, dev_action = a.dev_action;
    double* ma = reinterpret_cast<double*>(s_mem + sp.o_ma);
    double* mb = reinterpret_cast<double*>(s_mem + sp.o_mb);          // before the first step: reward_d, then dev_share's terms
    double* W = reinterpret_cast<double*>(s_mem + sp.o_w);
    double* Z = reinterpret_cast<double*>(s_mem + sp.o_z);
    double* Zd = reinterpret_cast<double*>(s_mem + a.o_zd);           // [D] the deviation step's Z
    uint16_t* first = reinterpret_cast<uint16_t*>(s_mem + sp.o_first);
    uint16_t* perm = reinterpret_cast<uint16_t*>(s_mem + sp.o_perm);
    uint16_t* ad = reinterpret_cast<uint16_t*>(s_mem + a.o_ad);       // [D] ad_g
    double* prod = reinterpret_cast<double*>(s_mem + sp.o_prod);      // [2N + 2][64] the chunk's terms per sum
    double* drow = reinterpret_cast<double*>(s_mem + a.o_dist);       // [64] the chunk's |x - x_0|
    SpCst* cst = reinterpret_cast<SpCst*>(s_mem + sp.o_cst);
    const int rb = a.row_begin, rc = a.row_count;

    sd_stage_grouping(sp, first, perm, tid);             // per config, staged once

    for (int64_t g = bid; g < G; g += nblk) {
        if (!sp_eps_ok(sp, g)) {                         // block-uniform: this game is not solved
            sd_unsolved(sp, a, g, tid);
            continue;
        }
        __syncthreads();                                 // the game before is read to its end; the grouping is staged
        const double* __restrict__ w0 = a.weights + g * T;

        // ---- the game's rows and constants, x_0 and the deviator's rewards
        sp_stage_game<1>(sp, s_mem, cst, g, tid);
        for (int t = tid; t < T; t += kSpBlock) {
            ma[t] = w0[t];
            mb[t] = sp.reward[(int64_t)dv * T + t];
        }
        __syncthreads();
        sp_normaliser(sp, s_mem, Z, tid);

        // ---- per price: ad_g and the deviation step's Z
        const uint16_t* devpol = a.use_policy ? a.dev_policy + g * D : nullptr;       // the game's row
        sd_price_strategy<MAXN>(sp, s_mem, cst, mb, ad, Zd, dv, dev_action, devpol, tid);
        __syncthreads();                                 // reward_d is read; ad_g of every price

        // ---- dev_share's terms over the dead second iterate (D <= T)
        sd_share_terms(sp, s_mem, cst, ma, first, perm, ad, mb, dv, tid);

        // ---- the baseline: what x_0 earns, and the share of periods the deviation changes
        double acc = sd_sums(sp, ma, w0, prod, drow, tid);       // its first barrier also ends the pass above
        const double base = acc;                         // lane 1 + i: base_reward_i
        sd_store_base(sp, a, acc, g, tid);
        if (tid == 64) {
            double s = 0.0;
            for (int d = 0; d < D; d++) s = __dadd_rn(s, mb[d]);
            a.dev_share[g] = s;
        }

        // ---- the deviator's row while the deviation lasts (every thread is past the barriers of the sums, so past its
        // reads of the own row)
        sd_replace_rows(sp, s_mem, cst, ad, dv, tid);
        __syncthreads();                                 // the terms are read before the second iterate is written

        // ---- K periods: the step x_{tau+1} = step_tau(x_tau), then the sums of x_{tau+1}
        const double gam = a.sweep_gamma ? a.sweep_gamma[(int64_t)dv * G + g] : a.gamma;
        SdTrack trk;
        double* mo = ma;
        double* mn = mb;
        for (int tau = 0; tau < K; tau++) {
            const bool dev = tau < L;
            if (tau == L) sp_stage_game<1>(sp, s_mem, cst, g, tid);     // the agents' own rows from here on
            sp_weights(sp, mo, first, perm, dev ? Zd : Z, W, tid);
            __syncthreads();
            for (int t = tid; t < T; t += kSpBlock) {
                int off[MAXN];
                sp_offsets<MAXN>(sp, t, off);
                mn[t] = sp_price_sum<MAXN>(sp, s_mem, cst, W, off);
            }
            __syncthreads();
            double* tm = mo; mo = mn; mn = tm;
            acc = sd_sums(sp, mo, w0, prod, drow, tid);
            sd_period(sp, a, trk, tau, acc, base, gam, dv, L, rb, rc, g, tid);
        }
        sd_finish(sp, a, trk, acc, dv, g, tid);
    }
}

#ifndef THRL_SP_HOST_BUILD
template <int MAXN>
__global__ void __launch_bounds__(kSpBlock) k_sd_chain(const SdArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    sd_block<MAXN>(a, s_mem, (int)threadIdx.x, (int)blockIdx.x, (int)gridDim.x);
}
#endif

}  // namespace

#ifndef THRL_SP_HOST_BUILD
int launch_sampled_deviation(const SdArgs& a, int grid, hipStream_t s) {
    return sp_launch(k_sd_chain<2>, k_sd_chain<kSpMaxA>, a, a.sp, grid, s);
}
#endif

}  // namespace thrl
