// thrl_sampled_deviation_noise.hip -- the deviation test of SAMPLED play UNDER DEMAND NOISE (thrl_sampled_deviation_noise,
// include/thrl_sampled_deviation_noise.h): thrl_sampled_deviation's impulse response in the environment of
// thrl_sampled_noise_chain.  The deviator conditions on the price, so its strategy ad_g lives on the S = D + Jn states, the
// distinct prices and then the quadrature nodes of a redrawn price.  One kernel.
//
// k_sdn_chain has k_sd_chain's shape: a 256-thread block per game, looping over games, everything but the networks' node
//   rows in LDS.  It joins two kernels and adds one pass.  A step is k_sd_chain's price half (sp_weights with the step's
//   Z, sp_price_sum over the staged rows, the deviator's written over while the deviation lasts: sd_replace_rows) plus
//   k_spn_chain's node half (spn_nu, then spn_node_pass, the streamed, double-buffered, register-staged tiles in
//   ascending j, thrl_sampled_noise_dev.h), Sn(t') parked in the iterate being written and x' = q Sd + p Sn by its owning
//   thread.  While the deviation lasts the node pass takes the deviator as deterministic (det): its node entries are the
//   uint16 row ad_g(D + j) in LDS, its probabilities 1.0 / 0.0 and Sn = 1.0, whatever its kind, and a network deviator's
//   tiles are neither loaded nor read.  The pass this kernel adds runs once per game before the first period
//   (sdn_node_setup): with every network's tile resident, one lane per node takes ad_g(D + j) -- for a best response the
//   first maximum over k of sr_q_of with U = Rn_delta, staged in the second iterate, which is dead until the first step, as
//   k_sd_chain stages reward_delta -- and parks dev_share's node term nu_0(j) * (1 - Pn_delta(ad|j) / Sn_delta(j)) over
//   nu_0(j) in V.  What this file keeps is the node setup, the order of a game's passes and the step; the staging of the
//   grouping, ad_g and Z at the prices (dev_policy's rows S long), dev_share's terms at the prices, the periods' sums (with
//   the noisy expectations), the bookkeeping on the lanes of the sums and the stores are the functions k_sd_chain calls
//   (thrl_sampled_deviation_dev.h).  No atomic is involved.  Nothing in the body is
//   wave-specific beyond spn_nu's THRL_SPN_WAVE_FIRST: with THRL_SP_HOST_BUILD the same source runs as 256 host threads
//   with barriers.
#include "thrl_response_dev.h"
#include "thrl_sampled_deviation_noise.h"
#include "thrl_sampled_deviation_dev.h"
#include "thrl_sampled_noise_dev.h"

namespace thrl {

namespace {

// Once per game, tile by tile in ascending j with every network's rows resident: ad_g(D + j) into adn[j], and dev_share's
// node term over nu_0(j) in V[j].  U holds Rn_delta; dv, dev_action and policy_row (the game's row of dev_policy from its
// entry of node 0 on, or NULL) as sd_price_strategy takes them.  Ends on a barrier.
template <int MAXN>
__device__ __forceinline__ void sdn_node_setup(const SpnArgs& na, unsigned char* s_mem, const SpCst* cst, const double* U, double* V,
                                               uint16_t* adn, int dv, int dev_action, const uint16_t* policy_row, int64_t g, int tid) {
    const SpArgs& sp = na.sp;
    const int N = sp.N, Jn = na.Jn, A = sp.n_actions[dv];
    const int n_tiles = (Jn + kSpnTile - 1) / kSpnTile;
    SpnWord st[MAXN][kSpnChunks];
    spn_tile_load<MAXN>(na, g, 0, tid, st);
    spn_tile_store<MAXN>(na, s_mem, 0, g, 0, tid, st);
    __syncthreads();
    for (int k = 0; k < n_tiles; k++) {
        const int j0 = k * kSpnTile, n = min(kSpnTile, Jn - j0), buf = k & 1;
        if (k + 1 < n_tiles) spn_tile_load<MAXN>(na, g, j0 + kSpnTile, tid, st);
        if (tid < n) {                                           // one lane per node
            const int j = j0 + tid;
            // Pn_i(x|j) from the resident tile, or a QTable agent's node entry
            auto prob = [&](int i, int x) THRL_SOLVE_INLINE {
                if (sp.kind[i] == 0) {
                    const uint16_t* nq = reinterpret_cast<const uint16_t*>(s_mem + na.o_nrow[i]);
                    return (int)nq[j] == x ? cst->hi[i] : cst->lo[i];
                }
                return (double)spn_tile_rows(na, s_mem, i, buf, g, j0)[tid * sp.n_actions[i] + x];
            };
            double zm = 1.0, Sown = 1.0;                         // Z_-delta(D + j) and Sn_delta(j)
            bool have = false;
            for (int i = 0; i < N; i++) {
                double Si = 1.0;
                if (sp.kind[i] != 0) {
                    Si = 0.0;
                    for (int x = 0; x < sp.n_actions[i]; x++) Si = __dadd_rn(Si, prob(i, x));
                }
                if (i == dv) { Sown = Si; continue; }
                zm = have ? __dmul_rn(zm, Si) : Si;
                have = true;
            }
            int act;
            if (policy_row) {
                act = min((int)policy_row[j], A - 1);
            } else if (dev_action >= 0) {
                act = dev_action;
            } else {                                             // the one-period best response at the node
                double bv;
                act = first_max(A, [&](int x) THRL_SOLVE_INLINE { return sr_q_of<MAXN>(sp, U, zm, dv, x, prob); }, bv);
            }
            adn[j] = (uint16_t)act;
            V[j] = __dmul_rn(V[j], __dsub_rn(1.0, __ddiv_rn(prob(dv, act), Sown)));
        }
        if (k + 1 < n_tiles) spn_tile_store<MAXN>(na, s_mem, buf ^ 1, g, j0 + kSpnTile, tid, st);
        __syncthreads();
    }
}

template <int MAXN>
__device__ __forceinline__ void sdn_block(const SdnArgs& a, unsigned char* s_mem, int tid, int bid, int nblk) {
    const SpnArgs& na = a.n;
    const SpArgs& sp = na.sp;
    const SdArgs& sd = a.sd;
    const int N = sp.N, G = sp.G, T = sp.T, D = sp.D, Jn = na.Jn, K = sd.K, L = sd.L, dv = sd.d, dev_action = sd.dev_action;
    double* ma = reinterpret_cast<double*>(s_mem + sp.o_ma);
    double* mb = reinterpret_cast<double*>(s_mem + sp.o_mb);          // before the first step: Rn_delta, then dev_share's terms
    double* W = reinterpret_cast<double*>(s_mem + sp.o_w);
    double* Z = reinterpret_cast<double*>(s_mem + sp.o_z);
    double* V = reinterpret_cast<double*>(s_mem + na.o_v);            // [Jn] nu, then V = nu / Zn tile by tile
    double* Zd = reinterpret_cast<double*>(s_mem + sd.o_zd);          // [D] the deviation step's Z
    uint16_t* first = reinterpret_cast<uint16_t*>(s_mem + sp.o_first);
    uint16_t* perm = reinterpret_cast<uint16_t*>(s_mem + sp.o_perm);
    uint16_t* ad = reinterpret_cast<uint16_t*>(s_mem + sd.o_ad);      // [D + Jn] ad_g: the prices, then the nodes
    double* prod = reinterpret_cast<double*>(s_mem + sp.o_prod);      // [2N + 2][64] the chunk's terms per sum
    double* drow = reinterpret_cast<double*>(s_mem + sd.o_dist);      // [64] the chunk's |x - x_0|
    SpCst* cst = reinterpret_cast<SpCst*>(s_mem + sp.o_cst);
    const int rb = sd.row_begin, rc = sd.row_count;

    sd_stage_grouping(sp, first, perm, tid);             // per config, staged once

    for (int64_t g = bid; g < G; g += nblk) {
        const double p = na.noise_prob_g ? na.noise_prob_g[g] : na.noise_prob;
        const double q = __dsub_rn(1.0, p);
        if (!(sp_eps_ok(sp, g) && p >= 0.0 && p <= 1.0)) {       // block-uniform: this game is not solved
            sd_unsolved(sp, sd, g, tid);
            continue;
        }
        __syncthreads();                                 // the game before is read to its end; the grouping is staged
        const double* __restrict__ w0 = sd.weights + g * T;

        // ---- the game's rows and constants, the QTable agents' entries at the nodes, x_0 and the deviator's Rn
        sp_stage_game<2>(sp, s_mem, cst, g, tid);
        for (int i = 0; i < N; i++)
            if (sp.kind[i] == 0) {
                uint16_t* nq = reinterpret_cast<uint16_t*>(s_mem + na.o_nrow[i]);
                const uint16_t* __restrict__ src = na.npolicy + (g * N + i) * Jn;
                for (int j = tid; j < Jn; j += kSpBlock) nq[j] = (uint16_t)min((int)src[j], sp.n_actions[i] - 1);
            }
        for (int t = tid; t < T; t += kSpBlock) {
            ma[t] = w0[t];
            mb[t] = __dadd_rn(__dmul_rn(q, sp.reward[(int64_t)dv * T + t]), __dmul_rn(p, na.noise_reward[(int64_t)dv * T + t]));
        }
        __syncthreads();
        sp_normaliser(sp, s_mem, Z, tid);
        spn_nu(na, ma, V, tid);                          // nu_0

        // ---- per price: ad_g and the deviation step's Z
        const uint16_t* devpol = sd.use_policy ? sd.dev_policy + g * (D + Jn) : nullptr;     // the game's row: prices, nodes
        sd_price_strategy<MAXN>(sp, s_mem, cst, mb, ad, Zd, dv, dev_action, devpol, tid);
        __syncthreads();                                 // nu_0 is whole
        // (ends on a barrier: Rn is read, ad_g is whole)
        sdn_node_setup<MAXN>(na, s_mem, cst, mb, V, ad + D, dv, dev_action, devpol ? devpol + D : nullptr, g, tid);

        // ---- dev_share's terms at the prices over the dead second iterate (D <= T)
        sd_share_terms(sp, s_mem, cst, ma, first, perm, ad, mb, dv, tid);

        // ---- the baseline: what x_0 earns, and the share of periods the deviation changes
        double acc = sd_sums<true>(sp, ma, w0, prod, drow, tid, q, p, na.noise_reward, na.noise_price);   // its first barrier also ends the pass above
        const double base = acc;                         // lane 1 + i: base_reward_i
        sd_store_base(sp, sd, acc, g, tid);
        if (tid == 64) {
            double s = 0.0;
            for (int d = 0; d < D; d++) s = __dadd_rn(s, mb[d]);
            cst->red[0] = s;
        } else if (tid == 128) {
            double s = 0.0;
            for (int j = 0; j < Jn; j++) s = __dadd_rn(s, V[j]);
            cst->red[1] = s;
        }

        // ---- the deviator's row at the prices while the deviation lasts (every thread is past the barriers of the sums,
        // so past its reads of the own row); at the nodes the pass takes ad_g as it stands
        sd_replace_rows(sp, s_mem, cst, ad, dv, tid);
        __syncthreads();                                 // the terms are read before the second iterate and V are written
        if (tid == 64) sd.dev_share[g] = __dadd_rn(__dmul_rn(q, cst->red[0]), __dmul_rn(p, cst->red[1]));

        // ---- K periods: the step x_{tau+1} = step_tau(x_tau), then the sums of x_{tau+1}
        const double gam = sd.sweep_gamma ? sd.sweep_gamma[(int64_t)dv * G + g] : sd.gamma;
        SdTrack trk;
        double* mo = ma;
        double* mn = mb;
        for (int tau = 0; tau < K; tau++) {
            const bool dev = tau < L;
            if (tau == L) sp_stage_game<2>(sp, s_mem, cst, g, tid);     // the agents' own rows from here on
            sp_weights(sp, mo, first, perm, dev ? Zd : Z, W, tid);
            spn_nu(na, mo, V, tid);
            __syncthreads();
            spn_node_pass<MAXN, true>(na, s_mem, cst, V, mn, false, g, tid, dev ? dv : -1, ad + D);   // Sn(t') into the iterate being written
            for (int t = tid; t < T; t += kSpBlock) {
                int off[MAXN];
                sp_offsets<MAXN>(sp, t, off);
                const double sdp = sp_price_sum<MAXN>(sp, s_mem, cst, W, off);
                mn[t] = __dadd_rn(__dmul_rn(q, sdp), __dmul_rn(p, mn[t]));
            }
            __syncthreads();
            double* tm = mo; mo = mn; mn = tm;
            acc = sd_sums<true>(sp, mo, w0, prod, drow, tid, q, p, na.noise_reward, na.noise_price);
            sd_period(sp, sd, trk, tau, acc, base, gam, dv, L, rb, rc, g, tid);
        }
        sd_finish(sp, sd, trk, acc, dv, g, tid);
    }
}

#ifndef THRL_SP_HOST_BUILD
template <int MAXN>
__global__ void __launch_bounds__(kSpBlock) k_sdn_chain(const SdnArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    sdn_block<MAXN>(a, s_mem, (int)threadIdx.x, (int)blockIdx.x, (int)gridDim.x);
}
#endif

}  // namespace

#ifndef THRL_SP_HOST_BUILD
int launch_sampled_deviation_noise(const SdnArgs& a, int grid, hipStream_t s) {
    return sp_launch(k_sdn_chain<2>, k_sdn_chain<kSpMaxA>, a, a.n.sp, grid, s);
}
#endif

}  // namespace thrl
