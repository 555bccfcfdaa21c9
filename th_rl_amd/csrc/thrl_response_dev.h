// thrl_response_dev.h -- the device functions k_sr_response (thrl_sampled_response.hip) and k_srn_response
// (thrl_sampled_response_noise.hip) share: a probability from the staged rows at the distinct prices; Q_V(s, k), the
// ordered sum over the tuples in which the agent plays k, for any state s whose rivals' probabilities the caller hands in
// as prob(j, x) = P_j(x|s); and what the two blocks do around their sweeps, over S states (the D prices, or the prices and
// then the nodes) with the probabilities as prob(j, s, k): the staging of the grouping (sr_stage_grouping), the outputs of
// a refused game or an unsolved agent (sr_flat_outputs), an agent's per-state setup (sr_setup_states), a solved state's
// stores (sr_store_state), the ordered loss sums over a range of states (sr_loss_range) and the four weighted sums
// (sr_weighted_sums).  The two calls name their scalar outputs differently: sr_flat and sr_summary have an overload per
// argument struct.  The sweeps themselves stay with their kernels (k_sr_response's team split, k_srn_response's one loop;
// the team rule of sr_layout stays with k_sr_response: with the node-states behind the prices k_srn_response always has
// more states than a team split serves).  Everything sits in namespace thrl's anonymous namespace, once per including
// file; with THRL_SP_HOST_BUILD the host harness supplies __device__, __syncthreads() and the rounded operations.
#pragma once
#include "thrl_sampled_dev.h"
#include "thrl_sampled_response.h"
#include "thrl_sampled_response_noise.h"
#include "thrl_solve_dev.h"

namespace thrl {

namespace {

// P_j(x|d) from the staged rows
__device__ __forceinline__ double sr_prob(const SpArgs& a, const unsigned char* s_mem, const SpCst* cst, int j, int d, int x) {
    if (a.kind[j] == 0) {
        const uint16_t* rq = reinterpret_cast<const uint16_t*>(s_mem + a.o_row[j]);
        return (int)rq[d] == x ? cst->hi[j] : cst->lo[j];
    }
    const float* rf = reinterpret_cast<const float*>(s_mem + a.o_row[j]);
    return (double)rf[d * a.n_actions[j] + x];
}

// Q_V(s, k) of agent i: sum over the tuples t with a_i(t) = k, ascending t from 0.0, of w(t|s) * U(t), divided by zm;
// prob(j, x) = P_j(x|s)
template <int MAXN, typename P>
__device__ __forceinline__ double sr_q_of(const SpArgs& a, const double* U, double zm, int i, int k, P prob) {
    const int N = a.N, T = a.T, A = a.n_actions[i], ts = a.tstride[i];
    double acc = 0.0;
    if (MAXN == 2 && N == 2) {                           // one rival: its action is the other digit of t
        const int r = 1 - i, Ar = a.n_actions[r];
        const int t0 = i == 0 ? k * Ar : k, dt = i == 0 ? 1 : A;
        for (int x = 0; x < Ar; x++) acc = __dadd_rn(acc, __dmul_rn(prob(r, x), U[t0 + x * dt]));
        return __ddiv_rn(acc, zm);
    }
    for (int base = k * ts; base < T; base += A * ts)
        for (int lo = 0; lo < ts; lo++) {
            const int t = base + lo;
            double w = 1.0;
            bool first = true;
            for (int j = 0; j < N; j++) {
                if (j == i) continue;
                const double p = prob(j, (t / a.tstride[j]) % a.n_actions[j]);
                w = first ? p : __dmul_rn(w, p);
                first = false;
            }
            acc = __dadd_rn(acc, __dmul_rn(w, U[t]));
        }
    return __ddiv_rn(acc, zm);
}

// Q_V(d, k) at the distinct price d, from the staged rows
template <int MAXN>
__device__ __forceinline__ double sr_q(const SpArgs& a, const unsigned char* s_mem, const SpCst* cst, const double* U, double zm,
                                       int i, int d, int k) {
    return sr_q_of<MAXN>(a, U, zm, i, k, [&](int j, int x) THRL_SOLVE_INLINE { return sr_prob(a, s_mem, cst, j, d, x); });
}

// the grouping of the tuples by price and row(t), the price of tuple t: per config, staged once; no entry leads out of
// bounds.  The caller synchronises before it reads trow.
__device__ __forceinline__ void sr_stage_grouping(const SpArgs& sp, uint16_t* first, uint16_t* perm, uint16_t* trow, int tid) {
    const int T = sp.T, D = sp.D;
    for (int d = tid; d <= D; d += kSpBlock) first[d] = (uint16_t)min(max(sp.grp_first[d], 0), T);
    for (int t = tid; t < T; t += kSpBlock) {
        perm[t] = (uint16_t)min(max(sp.grp_perm[t], 0), T - 1);
        trow[t] = 0;
    }
    __syncthreads();
    for (int d = tid; d < D; d += kSpBlock) {
        const int e = first[d + 1];
        for (int s = first[d]; s < e; s++) trow[perm[s]] = (uint16_t)d;
    }
}

// the scalar outputs the two calls name differently.  sr_flat: no state differs and every loss is x; sr_summary: the
// counts and the sums of sr_loss_range over the prices (nd, acc) and, under noise, over the nodes (ndn, accn)
__device__ __forceinline__ void sr_flat(const SrArgs& a, int64_t o, double x) {
    a.n_diff[o] = 0; a.loss_all[o] = x; a.loss_mean[o] = x;
}
__device__ __forceinline__ void sr_flat(const SrnArgs& a, int64_t o, double x) {
    a.n_diff_prices[o] = 0; a.n_diff_nodes[o] = 0; a.loss_all[o] = x; a.loss_prices_mean[o] = x; a.loss_nodes_mean[o] = x;
}
__device__ __forceinline__ void sr_summary(const SrArgs& a, int64_t o, double lmax, int nd, double acc, int, double) {
    a.n_diff[o] = nd; a.loss_all[o] = lmax; a.loss_mean[o] = __ddiv_rn(acc, (double)a.sp.D);
}
__device__ __forceinline__ void sr_summary(const SrnArgs& a, int64_t o, double lmax, int nd, double acc, int ndn, double accn) {
    a.n_diff_prices[o] = nd; a.n_diff_nodes[o] = ndn; a.loss_all[o] = lmax;
    a.loss_prices_mean[o] = __ddiv_rn(acc, (double)a.sp.D); a.loss_nodes_mean[o] = __ddiv_rn(accn, (double)a.Jn);
}

// the outputs of slot o over S states where nothing was solved: x = 0.0, no sweeps and the policy 0 (policy NULL) of a
// refused game; x = NaN, the sweeps made and the modal action of an unsolved (agent, game)
template <typename Args>
__device__ __forceinline__ void sr_flat_outputs(const Args& a, int64_t o, int S, double x, int sweeps, const uint16_t* policy,
                                                int tid) {
    if (tid == 0) {
        a.iters[o] = -1; a.sweeps[o] = sweeps;
        sr_flat(a, o, x);
        if (a.pi) { a.loss_w[o] = x; a.gain_w[o] = x; a.v_w[o] = x; a.br_prob_w[o] = x; }
    }
    for (int s = tid; s < S; s += kSpBlock) {
        if (a.br_policy) a.br_policy[o * S + s] = policy ? policy[s] : (uint16_t)0;
        if (a.v_opt) a.v_opt[o * S + s] = x;
        if (a.v_pi) a.v_pi[o * S + s] = x;
    }
}

// per state s of agent i: Z_-i(s), the product of the rivals' row sums, S_i(s), the agent's own, the modal action (a
// QTable agent's entry greedy(s), else the first maximum of its probabilities) into modal and sigma, and Va = 0;
// prob(j, s, k) = P_j(k|s)
template <typename P, typename Q>
__device__ __forceinline__ void sr_setup_states(const SpArgs& sp, int i, int S, double* Zm, double* Si, uint16_t* modal,
                                                uint16_t* sigma, double* Va, int tid, P prob, Q greedy) {
    const int N = sp.N, A = sp.n_actions[i];
    for (int s = tid; s < S; s += kSpBlock) {
        double z = 1.0, Sown = 1.0;
        bool have = false;
        for (int j = 0; j < N; j++) {
            double Sj = 1.0;
            if (sp.kind[j] != 0) {
                const int Aj = sp.n_actions[j];
                Sj = 0.0;
                for (int k = 0; k < Aj; k++) Sj = __dadd_rn(Sj, prob(j, s, k));
            }
            if (j == i) { Sown = Sj; continue; }
            z = have ? __dmul_rn(z, Sj) : Sj;
            have = true;
        }
        Zm[s] = z;
        Si[s] = Sown;
        int mo;
        if (sp.kind[i] == 0) {
            mo = greedy(s);
        } else {
            double bv;
            mo = first_max(A, [&](int k) THRL_SOLVE_INLINE { return prob(i, s, k); }, bv);
        }
        modal[s] = (uint16_t)mo;
        sigma[s] = (uint16_t)mo;
        Va[s] = 0.0;
    }
}

// a solved state's relative loss into loss[s], and its policy and values where they are stored
template <typename Args>
__device__ __forceinline__ void sr_store_state(const Args& a, int64_t o, int S, int s, const double* V, const double* Vpi,
                                               const uint16_t* sigma, double* loss) {
    const double vs = V[s], vp = Vpi[s];
    loss[s] = rel_loss(vs, vp);
    if (a.br_policy) a.br_policy[o * S + s] = sigma[s];
    if (a.v_opt) a.v_opt[o * S + s] = vs;
    if (a.v_pi) a.v_pi[o * S + s] = vp;
}

// one lane over the states [s0, s1) in ascending s: the largest loss so far, the ordered sum of the losses and the
// states where the best reply is not the modal action
__device__ __forceinline__ void sr_loss_range(const double* loss, const uint16_t* sigma, const uint16_t* modal, int s0, int s1,
                                              double& lmax, double& acc, int& nd) {
    for (int s = s0; s < s1; s++) {
        const double l = loss[s];
        if (l > lmax) lmax = l;
        acc = __dadd_rn(acc, l);
        nd += sigma[s] != modal[s] ? 1 : 0;
    }
}

// the four sums weighted by w(s), ordered over the S states: a lane of another wave than lane 0's for each;
// prob(s, k) = the agent's own P_i(k|s)
template <typename Args, typename P>
__device__ __forceinline__ void sr_weighted_sums(const Args& a, int64_t o, int S, const double* wgt, const double* loss,
                                                 const double* V, const double* Vpi, const double* Si, const uint16_t* sigma,
                                                 int tid, P prob) {
    if (tid >= 64 && tid < 68) {
        double acc = 0.0;
        for (int s = 0; s < S; s++) {
            const double w = wgt[s];
            double term;
            if (tid == 64) term = __dmul_rn(w, loss[s]);
            else if (tid == 65) term = __dmul_rn(w, __dsub_rn(V[s], Vpi[s]));
            else if (tid == 66) term = __dmul_rn(w, Vpi[s]);
            else term = __ddiv_rn(__dmul_rn(w, prob(s, sigma[s])), Si[s]);
            acc = __dadd_rn(acc, term);
        }
        (tid == 64 ? a.loss_w : tid == 65 ? a.gain_w : tid == 66 ? a.v_w : a.br_prob_w)[o] = acc;
    }
}

}  // namespace

}  // namespace thrl
