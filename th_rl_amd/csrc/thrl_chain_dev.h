// thrl_chain_dev.h -- the pieces the four long-run chain kernels share word for word: k_stationary (thrl_stationary.hip),
// k_ts_chain (thrl_tuple_stationary.hip), k_sp_chain (thrl_sampled.hip) and k_spn_chain (thrl_sampled_noise.hip).  Every
// one iterates m' = m / 2 + s / 2 per game and reports iters, change, mass, N rewards, N actions and a price, the sums
// taken in ascending order through product chunks [2N + 2][64] in LDS.  What is here: the outputs of a game that is not
// solved, one lazy update, the ordered read-back of a chunk and the final store.  The staging of the products and the
// block maximum stay in the kernels.  Device inline functions only, in namespace thrl's anonymous namespace, once per
// including file; no wave intrinsic, so with THRL_SP_HOST_BUILD the host harness supplies __device__ and the rounded
// operations as it does for thrl_sampled_dev.h.
#pragma once
#include <stdint.h>

namespace thrl {

namespace {

// game g is not solved: iters = -1 and zeros in every output; pi (may be NULL) has rows of `len` entries.  G and len are
// widened by the caller, once, as the kernels' own index arithmetic does
__device__ __forceinline__ void chain_unsolved(int32_t* iters, double* change, double* mass, double* price, double* reward,
                                               double* action, double* pi, int64_t g, int64_t G, int N, int64_t len, int tid,
                                               int block) {
    if (tid == 0) {
        iters[g] = -1;
        change[g] = 0.0;
        mass[g] = 0.0;
        price[g] = 0.0;
    }
    if (tid < N) {
        reward[tid * G + g] = 0.0;
        action[tid * G + g] = 0.0;
    }
    if (pi)
        for (int t = tid; t < len; t += block) pi[g * len + t] = 0.0;
}

// v = m / 2 + s / 2, with |v - m| folded into the thread's running maximum c
__device__ __forceinline__ double chain_lazy(double m, double s, double& c) {
    const double v = __dadd_rn(__dmul_rn(0.5, m), __dmul_rn(0.5, s));
    c = fmax(c, fabs(__dsub_rn(v, m)));
    return v;
}

// lane tid < n_out adds the n staged terms of its output (a row of kRow) in ascending order; the caller's barriers stand
// around it
template <int kRow = 64>
__device__ __forceinline__ double chain_read_back(const double* prod, int n_out, int n, double acc, int tid) {
    if (tid < n_out) {
        const double* pr = prod + tid * kRow;
        for (int kk = 0; kk < n; kk++) acc = __dadd_rn(acc, pr[kk]);
    }
    return acc;
}

// the final store, keyed by lane: 0 mass (with iters and change), 1 .. N rewards, N + 1 .. 2N actions, 2N + 1 price
__device__ __forceinline__ void chain_store(int32_t* iters, double* change, double* mass, double* price, double* reward,
                                            double* action, int64_t g, int G, int N, int tid, int it, double chg, double acc) {
    if (tid == 0) {
        iters[g] = it;
        change[g] = chg;
        mass[g] = acc;
    } else if (tid <= N) {
        reward[(int64_t)(tid - 1) * G + g] = acc;
    } else if (tid <= 2 * N) {
        action[(int64_t)(tid - 1 - N) * G + g] = acc;
    } else if (tid == 2 * N + 1) {
        price[g] = acc;
    }
}

}  // namespace

}  // namespace thrl
