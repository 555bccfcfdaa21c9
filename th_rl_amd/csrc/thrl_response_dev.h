// thrl_response_dev.h -- the device functions k_sr_response (thrl_sampled_response.hip) and k_srn_response
// (thrl_sampled_response_noise.hip) share: a probability from the staged rows at the distinct prices, and Q_V(s, k), the
// ordered sum over the tuples in which the agent plays k, for any state s whose rivals' probabilities the caller hands in
// as prob(j, x) = P_j(x|s).  (The team rule of sr_layout stays with k_sr_response: with the node-states behind the prices
// k_srn_response always has more states than a team split serves.)  Everything sits in namespace thrl's anonymous
// namespace, once per including file; with THRL_SP_HOST_BUILD the host harness supplies __device__ and the rounded
// operations.
#pragma once
#include "thrl_sampled_dev.h"
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

}  // namespace

}  // namespace thrl
