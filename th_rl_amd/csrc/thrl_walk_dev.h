// thrl_walk_dev.h -- the pieces the four kernels that walk a game's greedy map share word for word, one lane per game or
// match: k_deviation (thrl_deviation.hip) and k_xplay_walk (thrl_crossplay.hip), whose state is a row tuple int[MAXN]
// with N live entries, and k_tp_walk (thrl_tuple_play.hip) and k_ta_deviation (thrl_tuple_analysis.hip), whose state is
// one tuple index.  What is here: the cycle search, the copy and comparison of row tuples, the map on tuple indices,
// the means over the cycle, the zeroed outputs of a refused game, the store of a step into the row slice, the staged
// window of a policy with the scale-action LUT, and the copy of the reward / scaled tables into LDS.  The kernels'
// bodies, their maps and the sources of their staging loops stay in the kernels.  Device inline functions only, in
// namespace thrl's anonymous namespace, once per including file.  The search and the row helpers are integer code and
// __host__ __device__, so tests/walk_dev_check.cpp runs them on the host.
#pragma once
#include <stdint.h>

#include "thrl_device.h"

// on a lambda handed to these functions: inlined at every call, as the __forceinline__ functions around it are (the
// search applies its map in six places, and a map that stays a call puts the caller's row tuples into scratch)
#define THRL_WALK_INLINE __attribute__((always_inline))

namespace thrl {

namespace {

// ------------------------------------------------------------------------------------------------ the state of a walk
template <int MAXN>
__host__ __device__ __forceinline__ void copy_rows(int* dst, const int* src, int N) {
#pragma unroll
    for (int i = 0; i < MAXN; i++)
        if (i < N) dst[i] = src[i];
}

template <int MAXN>
__host__ __device__ __forceinline__ bool same_rows(const int* x, const int* y, int N) {
    bool e = true;
#pragma unroll
    for (int i = 0; i < MAXN; i++)
        if (i < N) e = e && x[i] == y[i];
    return e;
}

// a state is a row tuple (entries past N are neither read nor written) or one int
template <int MAXN>
__host__ __device__ __forceinline__ void copy_state(int (&dst)[MAXN], const int (&src)[MAXN], int N) { copy_rows<MAXN>(dst, src, N); }
__host__ __device__ __forceinline__ void copy_state(int& dst, const int& src, int) { dst = src; }

template <int MAXN>
__host__ __device__ __forceinline__ bool same_state(const int (&x)[MAXN], const int (&y)[MAXN], int N) { return same_rows<MAXN>(x, y, N); }
__host__ __device__ __forceinline__ bool same_state(const int& x, const int& y, int) { return x == y; }

// ------------------------------------------------------------------------------------------------ the cycle search
// Cycle of F from x0 within the horizon H (Brent, O(1) state); next(x) is x <- F(x).  Found iff mu + lam <= H: then
// s = x_mu.  Otherwise mu = H, lam = 0 and s = x_H (when want_s; else s is left alone).  Phase 1 stops at hare position
// 3H: if mu + lam <= H it detects the period by then (the tortoise sits at 2^k - 1 and detection comes at the first
// 2^k >= max(lam, mu + 1), so the hare is at 2^k - 1 + lam <= 3H - 2); phase 2 stops as soon as mu + lam would pass H.
// Every caller applies its map in this order, so a staged and a direct path take the same steps.
template <typename S, typename Next>
__host__ __device__ __forceinline__ bool find_cycle(const S& x0, int N, int H, Next next, int& mu, int& lam, S& s,
                                                    bool want_s) {
    S tort, hare;
    copy_state(tort, x0, N);
    copy_state(hare, x0, N);
    next(hare);
    int power = 1, l = 1, pos = 1;
    bool det = false;
    for (;;) {
        if (same_state(tort, hare, N)) { det = true; break; }
        if (pos >= 3 * H) break;
        if (power == l) { copy_state(tort, hare, N); power <<= 1; l = 0; }
        next(hare);
        l++;
        pos++;
    }
    bool found = det && l <= H;
    int m = 0;
    if (found) {
        copy_state(tort, x0, N);
        copy_state(hare, x0, N);
        for (int j = 0; j < l; j++) next(hare);
        while (!same_state(tort, hare, N)) {
            if (m + l >= H) { found = false; break; }
            next(tort);
            next(hare);
            m++;
        }
    }
    if (found) {
        mu = m;
        lam = l;
        copy_state(s, tort, N);
    } else {
        mu = H;
        lam = 0;
        if (want_s) {
            copy_state(s, x0, N);
            for (int j = 0; j < H; j++) next(s);
        }
    }
    return found;
}

// ------------------------------------------------------------------------------------------------ tuple indices
template <int MAXN>
struct TupleView {
    const uint16_t* gp[MAXN];       // agent i's T entries of the game it is taken from
};

// what agent i plays at tuple t: its entry clamped to its action count
template <int MAXN, typename A>
__device__ __forceinline__ int tuple_act(const A& a, const TupleView<MAXN>& v, int i, int t) {
    return min((int)v.gp[i][t], a.n_actions[i] - 1);
}

// F(t): the index of the tuple the agents play at t
template <int MAXN, typename A>
__device__ __forceinline__ int tuple_next(const A& a, const TupleView<MAXN>& v, int t) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < MAXN; i++)
        if (i < a.N) n += tuple_act<MAXN>(a, v, i, t) * a.tstride[i];
    return n;
}

// rew / sca <- copies of the [N][T] reward and scaled tables in LDS; every thread of the block calls it
__device__ __forceinline__ void stage_tables(unsigned char* s_mem, int n, int tid, int block, const double*& rew,
                                             const double*& sca) {
    double* tab = reinterpret_cast<double*>(s_mem);
    for (int j = tid; j < n; j += block) {
        tab[j] = rew[j];
        tab[n + j] = sca[j];
    }
    __syncthreads();
    rew = tab;
    sca = tab + n;
}

// ------------------------------------------------------------------------------------------------ outputs
// where one step's values lie: agent i's reward at rew[i * stride], its scaled action at sc[i * stride]
struct StepOut {
    const double* rew;
    const double* sc;
    int stride;
};

// cr, ca <- the mean reward and scaled action over the lam steps from the cycle's start; step() makes one transition
// of the caller's state and says where its values lie.  Sums from 0.0 in step order, one division; zeros when lam = 0.
// (k_xplay_walk keeps these lines inline: through this function its <gathered, 8> loses a wave per SIMD.)
template <int MAXN, typename Step>
__device__ __forceinline__ void cycle_means(int N, int lam, double* cr, double* ca, Step step) {
#pragma unroll
    for (int i = 0; i < MAXN; i++) { cr[i] = 0.0; ca[i] = 0.0; }
    if (lam > 0) {
        for (int j = 0; j < lam; j++) {
            const StepOut o = step();
#pragma unroll
            for (int i = 0; i < MAXN; i++)
                if (i < N) { cr[i] = __dadd_rn(cr[i], o.rew[i * o.stride]); ca[i] = __dadd_rn(ca[i], o.sc[i * o.stride]); }
        }
#pragma unroll
        for (int i = 0; i < MAXN; i++)
            if (i < N) { cr[i] = __ddiv_rn(cr[i], (double)lam); ca[i] = __ddiv_rn(ca[i], (double)lam); }
    }
}

// the means of game g of G
template <int MAXN, typename A>
__device__ __forceinline__ void store_means(const A& a, int64_t g, int64_t G, const double* cr, const double* ca) {
#pragma unroll
    for (int i = 0; i < MAXN; i++) {
        if (i >= a.N) break;
        a.cycle_reward[i * G + g] = cr[i];
        a.cycle_action[i * G + g] = ca[i];
    }
}

// step t of game g of G, where it lies in the slice [row_begin, row_begin + row_count) of the rows asked for
template <int MAXN, typename A>
__device__ __forceinline__ void store_step(const A& a, int t, int64_t g, int64_t G, const StepOut& o) {
    const int rr = t - a.row_begin;
    if (rr >= 0 && rr < a.row_count) {
#pragma unroll
        for (int i = 0; i < MAXN; i++) {
            if (i >= a.N) break;
            const int64_t at = (int64_t)rr * a.N * G + i * G + g;
            if (a.reward_rows) a.reward_rows[at] = o.rew[i * o.stride];
            if (a.action_rows) a.action_rows[at] = o.sc[i * o.stride];
        }
    }
}

// a refused game g of G: zeros in the means and in every row of the slice; mu, lam and the rest are the caller's
template <typename A>
__device__ __forceinline__ void store_refused(const A& a, int64_t g, int64_t G) {
    for (int i = 0; i < a.N; i++) {
        a.cycle_reward[i * G + g] = 0.0;
        a.cycle_action[i * G + g] = 0.0;
        for (int rr = 0; rr < a.row_count; rr++) {
            const int64_t at = (int64_t)rr * a.N * G + i * G + g;
            if (a.reward_rows) a.reward_rows[at] = 0.0;
            if (a.action_rows) a.action_rows[at] = 0.0;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the staged window
// A block stages, per game and agent, the win_n[i] rows from win_lo[i] the action grids can produce, then x_0's row:
// agent i's entries start at pol_off[i].
// the staged entry of agent i's row r: outside the window only x_0's row is visited
template <typename A>
__device__ __forceinline__ int window_entry(const A& a, int i, int r) {
    int k = r - a.win_lo[i];
    if ((unsigned)k >= (unsigned)a.win_n[i]) k = a.win_n[i];
    return a.pol_off[i] + k;
}

// the agent staged entry e belongs to
template <typename A>
__device__ __forceinline__ int window_agent(const A& a, int e) {
    int i = 0;
    while (i + 1 < a.N && e >= a.pol_off[i + 1]) i++;
    return i;
}

// the table row staged entry e of agent i stands for, in a game that starts at price st (read for x_0's row only)
template <typename A>
__device__ __forceinline__ int window_row(const A& a, int i, int e, const double& st) {
    const int k = e - a.pol_off[i];
    return k < a.win_n[i] ? a.win_lo[i] + k : encode64_fast(st, a.ag[i]);
}

// lut <- every agent's scaled actions, agent i's from lut_off[i]; the caller synchronises before the walk reads them
template <typename A>
__device__ __forceinline__ void fill_scale_lut(const A& a, double* lut, int tid, int block) {
    for (int j = tid; j < a.lut_n; j += block) {
        int i = 0;
        while (i + 1 < a.N && j >= a.lut_off[i + 1]) i++;
        lut[j] = scale_action(j - a.lut_off[i], a.ag[i]);
    }
}

}  // namespace

}  // namespace thrl
