// thrl_tuple_play.hip -- strategies as tables over the game's action tuples, and greedy play on tuple indices
// (thrl_tuple_policy, thrl_tuple_walk, include/thrl.h).  With discrete agents and no noise the price after a step is a
// function of that step's action tuple, so what any agent does next is a function of the tuple index: a uint16 per
// (game, agent, tuple), whatever the agent is.  Four kernels.
//
// k_tp_neural: one wavefront per game for ONE Reinforce / ActorCritic agent (a launch per neural agent, so the
//   register-resident network is sized for that agent's action count, as k_nn_act's is).  policy_load puts the
//   weights in registers once; the T prices come in runs of 64, one per lane, and are handed to the whole wave by
//   v_readlane, so the evaluation loop touches no memory.  Lane j keeps the action of the run's j-th price and the
//   wave stores the run as one contiguous 128-byte piece.  The evaluation is thrl_policy.h's policy_act, the function
//   k_nn_act calls, with the same padding: the same bits.
//   thrl_price_policy runs the same kernels on a free list of J prices, shared by the games or one list per game
//   (price_stride): T stands for J there.
// k_tp_probs: k_tp_neural's loop storing the probabilities themselves (thrl_price_probs): float32 [G][J][A].
// k_tp_qtable: one thread per (game, tuple), every QTable agent in turn: the first maximum of row encode64(price[t]).
//   Consecutive tuples have neighbouring prices, so a wave reads a few neighbouring rows and its stores are contiguous.
// k_tp_walk: one lane per match, the walk of k_xplay_walk on a single integer.  The 2-byte policy entries it visits
//   are gathered from global memory (mu + lam is a handful of steps); the per-config reward and scaled-action tables
//   sit in LDS when they fit kTpLdsBudget.  The map on tuple indices, the cycle search, the means over the cycle, the
//   refused match's zeros, the store of the row slice and the staging of the tables are thrl_walk_dev.h's.
#include "thrl_tuple_play.h"

#include "thrl_policy.h"
#include "thrl_walk_dev.h"

namespace thrl {

namespace {

// ------------------------------------------------------------------------------------------------ extraction
template <int APAD>
__global__ void __launch_bounds__(256) k_tp_neural(int G, int A, int T, const float* __restrict__ params, int P,
                                                    const double* __restrict__ price, int64_t price_stride,
                                                    uint16_t* __restrict__ out, int64_t out_stride) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= G) return;
    PolicyRegs<APAD> r;
    policy_load(r, params + (int64_t)g * P, A, lane);
    uint16_t* o = out + (int64_t)g * out_stride;
    price += (int64_t)g * price_stride;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int n = T - t0 < 64 ? T - t0 : 64;
        const float xv = (float)price[t0 + (lane < n ? lane : n - 1)];
        int keep = 0;
        for (int j = 0; j < n; j++) {
            const float x = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, xv), j));
            const int act = policy_act(r, A, x, false, 0.0f, lane, nullptr);
            if (lane == j) keep = act;
        }
        if (lane < n) o[t0 + lane] = (uint16_t)keep;
    }
}

// the probabilities where k_tp_neural keeps the action (thrl_price_probs): policy_probs, the function policy_act calls
// first, with the network in registers across the J shared prices; lane 2k holds action k's probability and stores it,
// so a price's row leaves the wave as one contiguous piece of A floats
template <int APAD>
__global__ void __launch_bounds__(256) k_tp_probs(int G, int A, int J, const float* __restrict__ params, int P,
                                                   const double* __restrict__ price, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= G) return;
    PolicyRegs<APAD> r;
    policy_load(r, params + (int64_t)g * P, A, lane);
    float* o = out + (int64_t)g * J * A;
    const bool mine = !(lane & 1) && (lane >> 1) < A;
    for (int t0 = 0; t0 < J; t0 += 64) {
        const int n = J - t0 < 64 ? J - t0 : 64;
        const float xv = (float)price[t0 + (lane < n ? lane : n - 1)];
        for (int j = 0; j < n; j++) {
            const float x = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, xv), j));
            const float p = policy_probs(r, A, x, lane);
            if (mine) o[(int64_t)(t0 + j) * A + (lane >> 1)] = p;
        }
    }
}

template <typename Tq>
__global__ void __launch_bounds__(256) k_tp_qtable(const TpPolicyArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)a.G * a.T) return;
    const int64_t g = idx / a.T;
    const int t = (int)(idx - g * a.T);
    const double p = a.price[g * a.price_stride + t];
    const Tq* __restrict__ q = reinterpret_cast<const Tq*>(a.q) + g * a.stride;
    for (int j = 0; j < a.n_q; j++) {
        const int i = a.q_agent[j];
        const AgentParams& ag = a.ag[i];
        const int row = encode64(p, ag);
        a.policy[(g * a.N + i) * a.T + t] = (uint16_t)argmax_row(q + ag.table_off + (int64_t)row * ag.n_actions, ag.n_actions);
    }
}

// ------------------------------------------------------------------------------------------------ walk
template <bool kLds, int MAXN>
__global__ void __launch_bounds__(kTpTile) k_tp_walk(const TpWalkArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    const int tid = threadIdx.x;
    const int M = a.M, N = a.N, T = a.T;
    const double* rew = a.reward;
    const double* sca = a.scaled;
    if constexpr (kLds) stage_tables(s_mem, N * T, tid, kTpTile, rew, sca);
    const int64_t m = (int64_t)blockIdx.x * kTpTile + tid;
    if (m >= M) return;

    TupleView<MAXN> v;              // the seated games' entries
    bool ok = true;
#pragma unroll
    for (int i = 0; i < MAXN; i++) {
        if (i >= N) break;
        const int64_t g = a.seat[(int64_t)i * M + m];
        const bool in = g >= 0 && g < a.G;
        ok = ok && in;
        v.gp[i] = a.policy + ((in ? g : 0) * N + i) * T;
    }
    const int t0 = a.start[m];
    ok = ok && t0 >= 0 && t0 < T;
    if (!ok) {                                          // the stated sentinel: mu = -1, lam = 0 and zeros
        a.mu[m] = -1;
        a.lam[m] = 0;
        if (a.cycle_start) a.cycle_start[m] = -1;
        store_refused(a, m, M);
        return;
    }

    // t <- the index of the tuple the seated agents play at t, and where the values of that tuple lie
    const auto next = [&](int& t) THRL_WALK_INLINE {
        t = tuple_next<MAXN>(a, v, t);
        return StepOut{rew + t, sca + t, T};
    };
    int mu, lam, s = 0;
    find_cycle(t0, N, a.H, next, mu, lam, s, false);
    double cr[MAXN], ca[MAXN];
    int x = s;
    cycle_means<MAXN>(N, lam, cr, ca, [&]() THRL_WALK_INLINE { return next(x); });
    a.mu[m] = mu;
    a.lam[m] = lam;
    if (a.cycle_start) a.cycle_start[m] = lam > 0 ? s : -1;
    store_means<MAXN>(a, m, M, cr, ca);

    // the path from t_0: the rows of tau in [row_begin, row_begin + row_count)
    if (a.row_count > 0 && (a.reward_rows || a.action_rows)) {
        x = t0;
        const int end = a.row_begin + a.row_count;
        for (int tau = 0; tau < end; tau++) store_step<MAXN>(a, tau, m, M, next(x));
    }
}

template <bool kLds>
void launch_walk_n(const TpWalkArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)(((int64_t)a.M + kTpTile - 1) / kTpTile)), block(kTpTile);
    const size_t lds = (size_t)a.lds_bytes;
    if (a.N <= 2) hipLaunchKernelGGL((k_tp_walk<kLds, 2>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((k_tp_walk<kLds, THRL_MAXA>), grid, block, lds, s, a);
}

}  // namespace

int launch_tp_policy(const TpPolicyArgs& a, int q_dtype, hipStream_t s) {
    if (a.n_q > 0) {
        const int64_t n = (int64_t)a.G * a.T;
        const dim3 grid((unsigned)((n + 255) / 256)), block(256);
        if (q_dtype == 1) hipLaunchKernelGGL(k_tp_qtable<double>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(k_tp_qtable<float>, grid, block, 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    for (int j = 0; j < a.n_nn; j++) {
        const dim3 grid((unsigned)((a.G + 3) / 4)), block(256);
        const int A = a.nn_actions[j];
        uint16_t* out = a.policy + (int64_t)a.nn_agent[j] * a.T;
        const int64_t os = (int64_t)a.N * a.T;
        // the padding k_nn_act takes for this action count
        if (A <= 8) hipLaunchKernelGGL(k_tp_neural<8>, grid, block, 0, s, a.G, A, a.T, a.nn_params[j], a.nn_stride[j], a.price, a.price_stride, out, os);
        else if (A <= 24) hipLaunchKernelGGL(k_tp_neural<24>, grid, block, 0, s, a.G, A, a.T, a.nn_params[j], a.nn_stride[j], a.price, a.price_stride, out, os);
        else hipLaunchKernelGGL(k_tp_neural<32>, grid, block, 0, s, a.G, A, a.T, a.nn_params[j], a.nn_stride[j], a.price, a.price_stride, out, os);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return (int)hipSuccess;
}

int launch_tp_probs(int G, int A, int J, const float* params, int P, const double* price, float* out, hipStream_t s) {
    const dim3 grid((unsigned)((G + 3) / 4)), block(256);
    // the padding k_nn_act takes for this action count
    if (A <= 8) hipLaunchKernelGGL(k_tp_probs<8>, grid, block, 0, s, G, A, J, params, P, price, out);
    else if (A <= 24) hipLaunchKernelGGL(k_tp_probs<24>, grid, block, 0, s, G, A, J, params, P, price, out);
    else hipLaunchKernelGGL(k_tp_probs<32>, grid, block, 0, s, G, A, J, params, P, price, out);
    return (int)hipGetLastError();
}

int launch_tp_walk(const TpWalkArgs& a, hipStream_t s) {
    if (a.in_lds) launch_walk_n<true>(a, s);
    else launch_walk_n<false>(a, s);
    return (int)hipGetLastError();
}

}  // namespace thrl
