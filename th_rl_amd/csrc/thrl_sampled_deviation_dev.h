// thrl_sampled_deviation_dev.h -- what the two deviation tests of sampled play, k_sd_chain (thrl_sampled_deviation.hip)
// and k_sdn_chain (thrl_sampled_deviation_noise.hip), have in common, once: the staging of the grouping
// (sd_stage_grouping), a row sum from the staged rows (sd_row_sum), the outputs of an unsolved game (sd_unsolved), the
// deviator's strategy at the distinct prices with the deviation step's Z (sd_price_strategy; it takes the game's row of
// dev_policy, D long there and D + Jn here), dev_share's terms at the prices (sd_share_terms), the ordered sums of a
// distribution (sd_sums, with the noisy expectations for k_sdn_chain), the baseline's stores (sd_store_base), the
// replacement of the deviator's staged rows (sd_replace_rows) and what the lanes of the sums derive over the periods
// (SdTrack, sd_period, sd_finish).  Both kernels call every one of them; what stays with a kernel is its step and, in
// k_sdn_chain, the nodes.  The functions take the SpArgs they read beside the SdArgs, so that k_sdn_chain, whose SpArgs
// sits in its SpnArgs, passes that one.  What a function needs of SdArgs' first run of fields -- the deviator, dev_len,
// dev_action -- and the row range come by value, read once at the top of the caller's block function, and the strategy
// functions take the game's row of dev_policy (or NULL), not the struct: a function that reads a.d or a.dev_action itself
// has the run loaded again where it is inlined, and the compiler keeps a stack slot for the tuple it spills whole (20
// bytes of scratch reserved, never accessed: in k_sd_chain<2> and <8> with sd_price_strategy reading a.d, in
// k_sdn_chain<8> with it reading a.dev_action).  As it stands no kernel has scratch, k_sd_chain has 103 / 121 VGPRs and
// the parent's 4 waves per SIMD (profiles/deviation_shared_resource_usage.txt), and its rate is the parent's
// (profiles/deviation_shared.md).  Everything sits in namespace thrl's anonymous namespace, once per including file; with
// THRL_SP_HOST_BUILD the host harness supplies __device__, __syncthreads() and the rounded operations.
#pragma once
#include "thrl_response_dev.h"
#include "thrl_sampled_deviation.h"
#include "thrl_sampled_dev.h"

namespace thrl {

namespace {

// the grouping of the tuples by price: per config, staged once; no entry leads out of bounds
__device__ __forceinline__ void sd_stage_grouping(const SpArgs& sp, uint16_t* first, uint16_t* perm, int tid) {
    const int T = sp.T, D = sp.D;
    for (int d = tid; d <= D; d += kSpBlock) first[d] = (uint16_t)min(max(sp.grp_first[d], 0), T);
    for (int t = tid; t < T; t += kSpBlock) perm[t] = (uint16_t)min(max(sp.grp_perm[t], 0), T - 1);
}

// S_j(d) from the staged rows
__device__ __forceinline__ double sd_row_sum(const SpArgs& sp, const unsigned char* s_mem, int j, int d) {
    if (sp.kind[j] == 0) return 1.0;
    const int A = sp.n_actions[j];
    const float* rf = reinterpret_cast<const float*>(s_mem + sp.o_row[j]) + d * A;
    double S = 0.0;
    for (int k = 0; k < A; k++) S = __dadd_rn(S, (double)rf[k]);
    return S;
}

// game g is not solved: zeros in every float64 output, its rows included, and -1 in low_step and ret_step
__device__ __forceinline__ void sd_unsolved(const SpArgs& sp, const SdArgs& a, int64_t g, int tid) {
    const int N = sp.N, G = sp.G, rc = a.row_count;
    if (tid < N) {
        a.base_reward[(int64_t)tid * G + g] = 0.0;
        a.base_action[(int64_t)tid * G + g] = 0.0;
    }
    if (tid == 0) {
        a.base_price[g] = 0.0; a.dev_share[g] = 0.0; a.gain[g] = 0.0; a.gain_dev[g] = 0.0; a.low[g] = 0.0; a.dist[g] = 0.0;
        a.mass[g] = 0.0; a.low_step[g] = -1; a.ret_step[g] = -1;
    }
    for (int r = tid; r < rc * N; r += kSpBlock) {
        if (a.reward_rows) a.reward_rows[(int64_t)r * G + g] = 0.0;
        if (a.action_rows) a.action_rows[(int64_t)r * G + g] = 0.0;
    }
    for (int r = tid; r < rc; r += kSpBlock) {
        if (a.price_rows) a.price_rows[(int64_t)r * G + g] = 0.0;
        if (a.dist_rows) a.dist_rows[(int64_t)r * G + g] = 0.0;
    }
}

// per price, a thread each: ad_g(d) into ad -- the entry of policy_row, the game's row of dev_policy (clamped) or NULL; else
// dev_action where it is one; else the one-period best response to the rivals' mixed policies, the first maximum over k of
// sr_q with U the deviator's rewards -- and the deviation step's Z(d), the product with S_d = 1.0, into Zd
template <int MAXN>
__device__ __forceinline__ void sd_price_strategy(const SpArgs& sp, const unsigned char* s_mem, const SpCst* cst, const double* U,
                                                  uint16_t* ad, double* Zd, int dv, int dev_action, const uint16_t* policy_row,
                                                  int tid) {
    const int N = sp.N, D = sp.D, A = sp.n_actions[dv];
    for (int d = tid; d < D; d += kSpBlock) {
        double zm = 1.0, zd = 1.0;                       // Z_-d and Z with S_d = 1.0
        bool have = false;
        for (int j = 0; j < N; j++) {
            const double Sj = j == dv ? 1.0 : sd_row_sum(sp, s_mem, j, d);
            zd = j == 0 ? Sj : __dmul_rn(zd, Sj);
            if (j == dv) continue;
            zm = have ? __dmul_rn(zm, Sj) : Sj;
            have = true;
        }
        int act;
        if (policy_row) {
            act = min((int)policy_row[d], A - 1);
        } else if (dev_action >= 0) {
            act = dev_action;
        } else {
            double bv;
            act = first_max(A, [&](int k) THRL_SOLVE_INLINE { return sr_q<MAXN>(sp, s_mem, cst, U, zm, dv, d, k); }, bv);
        }
        ad[d] = (uint16_t)act;
        Zd[d] = zd;
    }
}

// dev_share's terms at the prices, M_0(d) * (1 - P_d(ad_g(d)|d) / S_d(d)) with M_0 the mass of m at price d, into out[d]
__device__ __forceinline__ void sd_share_terms(const SpArgs& sp, const unsigned char* s_mem, const SpCst* cst, const double* m,
                                               const uint16_t* first, const uint16_t* perm, const uint16_t* ad, double* out, int dv,
                                               int tid) {
    const int D = sp.D;
    for (int d = tid; d < D; d += kSpBlock) {
        double M = 0.0;
        const int e = first[d + 1];
        for (int s = first[d]; s < e; s++) M = __dadd_rn(M, m[perm[s]]);
        const double own = __ddiv_rn(sr_prob(sp, s_mem, cst, dv, d, (int)ad[d]), sd_row_sum(sp, s_mem, dv, d));
        out[d] = __dmul_rn(M, __dsub_rn(1.0, own));
    }
}

// the ordered sums of one distribution m against x_0 = w0; lane o <= 2N + 2 its own: 0 the mass, 1 .. N the rewards,
// N + 1 .. 2N the actions, 2N + 1 the price, 2N + 2 the sum of |m - x_0| (staged in drow).  NOISE: the rewards and the
// price are the expectations under demand noise, q * reward_i(t) + p * nreward_i(t) and q * price(t) + p * nprice(t)
template <bool NOISE = false>
__device__ __forceinline__ double sd_sums(const SpArgs& sp, const double* m, const double* __restrict__ w0, double* prod,
                                          double* drow, int tid, double q = 1.0, double p = 0.0,
                                          const double* __restrict__ nreward = nullptr, const double* __restrict__ nprice = nullptr) {
    const int N = sp.N, T = sp.T, n_out = 2 * N + 2;
    double acc = 0.0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + tid;
        if (tid < 64 && t < T) {
            const double mt = m[t];
            prod[tid] = mt;
            for (int i = 0; i < N; i++) {
                double r = sp.reward[(int64_t)i * T + t];
                if (NOISE) r = __dadd_rn(__dmul_rn(q, r), __dmul_rn(p, nreward[(int64_t)i * T + t]));
                prod[(1 + i) * 64 + tid] = __dmul_rn(mt, r);
                prod[(1 + N + i) * 64 + tid] = __dmul_rn(mt, sp.scaled[(int64_t)i * T + t]);
            }
            double pr = sp.price[t];
            if (NOISE) pr = __dadd_rn(__dmul_rn(q, pr), __dmul_rn(p, nprice[t]));
            prod[(1 + 2 * N) * 64 + tid] = __dmul_rn(mt, pr);
            drow[tid] = fabs(__dsub_rn(mt, w0[t]));
        }
        __syncthreads();
        const int n = min(64, T - t0);
        acc = tid == n_out ? chain_read_back(drow, 1, n, acc, 0) : chain_read_back(prod, n_out, n, acc, tid);
        __syncthreads();
    }
    return acc;
}

// What the lanes of the sums keep over the periods: lane 1 + delta the gain and the low, lane 2 N + 2 the distance and
// ret_step (the other lanes carry the fields unused)
struct SdTrack {
    double w = 1.0, gain = 0.0, gain_dev = 0.0, low = 0.0, Dist = 0.0;
    int low_step = -1, ret = -1;
};

// period tau's bookkeeping from its sums (acc, sd_sums' lane value) against the baseline's (base), and its rows; dv, L, rb
// and rc are a.d, a.L, a.row_begin and a.row_count, read once by the caller
__device__ __forceinline__ void sd_period(const SpArgs& sp, const SdArgs& a, SdTrack& k, int tau, double acc, double base,
                                          double gam, int dv, int L, int rb, int rc, int64_t g, int tid) {
    const int N = sp.N, G = sp.G, n_out = 2 * N + 2;
    const bool dev = tau < L;
    k.Dist = __dmul_rn(0.5, acc);                        // the distance, on lane n_out
    if (tid == 1 + dv) {
        const double diff = __dsub_rn(acc, base);
        const double term = __dmul_rn(k.w, diff);
        k.gain = __dadd_rn(k.gain, term);
        if (dev) {
            k.gain_dev = __dadd_rn(k.gain_dev, term);
        } else if (tau == L || diff < k.low) {
            k.low = diff;
            k.low_step = tau;
        }
        k.w = __dmul_rn(k.w, gam);
    }
    if (tid == n_out && !dev && k.ret < 0 && k.Dist <= a.ret_tol) k.ret = tau;
    const int r = tau - rb;
    if (r >= 0 && r < rc) {
        if (tid >= 1 && tid <= N) {
            if (a.reward_rows) a.reward_rows[((int64_t)r * N + (tid - 1)) * G + g] = acc;
        } else if (tid > N && tid <= 2 * N) {
            if (a.action_rows) a.action_rows[((int64_t)r * N + (tid - 1 - N)) * G + g] = acc;
        } else if (tid == 2 * N + 1) {
            if (a.price_rows) a.price_rows[(int64_t)r * G + g] = acc;
        } else if (tid == n_out) {
            if (a.dist_rows) a.dist_rows[(int64_t)r * G + g] = k.Dist;
        }
    }
}

// the per-game outputs after the last period (acc: its sums)
__device__ __forceinline__ void sd_finish(const SpArgs& sp, const SdArgs& a, const SdTrack& k, double acc, int dv, int64_t g,
                                          int tid) {
    if (tid == 1 + dv) {
        a.gain[g] = k.gain; a.gain_dev[g] = k.gain_dev; a.low[g] = k.low; a.low_step[g] = k.low_step;
    } else if (tid == 2 * sp.N + 2) {
        a.ret_step[g] = k.ret; a.dist[g] = k.Dist;
    } else if (tid == 0) {
        a.mass[g] = acc;
    }
}

// the baseline's stores: lane 1 + i base_reward_i, lane 1 + N + i base_action_i, lane 2 N + 1 base_price
__device__ __forceinline__ void sd_store_base(const SpArgs& sp, const SdArgs& a, double acc, int64_t g, int tid) {
    const int N = sp.N, G = sp.G;
    if (tid >= 1 && tid <= N) a.base_reward[(int64_t)(tid - 1) * G + g] = acc;
    else if (tid > N && tid <= 2 * N) a.base_action[(int64_t)(tid - 1 - N) * G + g] = acc;
    else if (tid == 2 * N + 1) a.base_price[g] = acc;
}

// the deviator's staged rows at the distinct prices while the deviation lasts: P_d(k|d) = 1.0 for k = ad(d), else 0.0
__device__ __forceinline__ void sd_replace_rows(const SpArgs& sp, unsigned char* s_mem, SpCst* cst, const uint16_t* ad, int dv,
                                                int tid) {
    const int D = sp.D, A = sp.n_actions[dv];
    if (sp.kind[dv] == 0) {
        uint16_t* rq = reinterpret_cast<uint16_t*>(s_mem + sp.o_row[dv]);
        for (int d = tid; d < D; d += kSpBlock) rq[d] = ad[d];
        if (tid == 0) { cst->hi[dv] = 1.0; cst->lo[dv] = 0.0; }
    } else {
        float* rf = reinterpret_cast<float*>(s_mem + sp.o_row[dv]);
        for (int d = tid; d < D; d += kSpBlock) {
            const int act = ad[d];
            for (int k = 0; k < A; k++) rf[d * A + k] = k == act ? 1.0f : 0.0f;
        }
    }
}

}  // namespace

}  // namespace thrl
