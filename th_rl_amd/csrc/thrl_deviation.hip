// thrl_deviation.hip -- deviation analysis of the greedy policies (thrl_deviation, include/thrl.h): the limit
// cycle of greedy play, a forced deviation of one agent, the response of the others, the discounted gain of the
// deviator and whether play returns to the cycle.  One lane per game.
//
// Staged path: the block first stages every game's greedy policy into LDS -- the argmax of each row the walk can
// reach (the window of rows the action grids can produce, plus x_0's row), one byte or two per entry -- and a LUT
// of every agent's scaled actions.  The walk then needs no table reads and no division in scale_action.  Configs
// whose policy does not fit kDevLdsBudget take the direct path, which reads each visited row from HBM.  Both walk
// the same map with the same operations, so both give the same bits.
#include "thrl_deviation.h"

namespace thrl {

namespace {

template <typename T, typename P, bool kStaged>
struct View {                   // where a lane finds its game's greedy policy
    const T* __restrict__ qg;   // direct: the game's tables
    const P* pol;               // staged: entry e of this lane's game at pol[e * kDevTile]
    const double* lut;          // staged: scaled actions, agent i's at lut[lut_off[i] ..]
};

template <typename T, typename P, bool kStaged>
__device__ __forceinline__ int policy(const DevArgs& a, const View<T, P, kStaged>& v, int i, int r) {
    if constexpr (kStaged) {
        int k = r - a.win_lo[i];
        if ((unsigned)k >= (unsigned)a.win_n[i]) k = a.win_n[i];      // outside the window only x_0's row is visited
        return (int)v.pol[(a.pol_off[i] + k) * kDevTile];
    } else {
        const AgentParams& p = a.ag[i];
        return argmax_row(v.qg + p.table_off + (int64_t)r * p.n_actions, p.n_actions);
    }
}

template <typename T, typename P, bool kStaged>
__device__ __forceinline__ double scaled_of(const DevArgs& a, const View<T, P, kStaged>& v, int i, int act) {
    if constexpr (kStaged) return v.lut[a.lut_off[i] + act];
    else return scale_action(act, a.ag[i]);
}

template <int MAXN>
__device__ __forceinline__ void copy_rows(int* dst, const int* src, int N) {
#pragma unroll
    for (int i = 0; i < MAXN; i++)
        if (i < N) dst[i] = src[i];
}

template <int MAXN>
__device__ __forceinline__ bool same_rows(const int* x, const int* y, int N) {
    bool e = true;
#pragma unroll
    for (int i = 0; i < MAXN; i++)
        if (i < N) e = e && x[i] == y[i];
    return e;
}

template <int MAXN>
__device__ __forceinline__ double pick(const double* v, int d, int N) {     // v[d] without a dynamic register index
    double r = 0.0;
#pragma unroll
    for (int i = 0; i < MAXN; i++)
        if (i < N && i == d) r = v[i];
    return r;
}

// One transition from the state whose actions are act[]: scaled actions, rewards, and the next rows into x.
template <typename T, typename P, bool kStaged, int MAXN>
__device__ __forceinline__ void transition(const DevArgs& a, const View<T, P, kStaged>& v, const int* act, double* sc,
                                           double* rew, int* x) {
    const int N = a.N;
#pragma unroll
    for (int i = 0; i < MAXN; i++)
        if (i < N) sc[i] = scaled_of(a, v, i, act[i]);
    const double p = env_step<MAXN>(a.env, N, sc, a.env.a, rew);
#pragma unroll
    for (int i = 0; i < MAXN; i++)
        if (i < N) x[i] = encode64_fast(p, a.ag[i]);
}

template <typename T, typename P, bool kStaged, int MAXN>
__device__ __forceinline__ void greedy_actions(const DevArgs& a, const View<T, P, kStaged>& v, const int* x, int* act) {
#pragma unroll
    for (int i = 0; i < MAXN; i++)
        if (i < a.N) act[i] = policy(a, v, i, x[i]);
}

// x <- F(x): the greedy map on row tuples
template <typename T, typename P, bool kStaged, int MAXN>
__device__ __forceinline__ void greedy_map(const DevArgs& a, const View<T, P, kStaged>& v, int* x) {
    int act[MAXN];
    double sc[MAXN], rew[MAXN];
    greedy_actions<T, P, kStaged, MAXN>(a, v, x, act);
    transition<T, P, kStaged, MAXN>(a, v, act, sc, rew, x);
}

// Cycle of F from x0 within the horizon H (Brent, O(1) state).  Found iff mu + lam <= H: then s = x_mu.  Otherwise
// mu = H, lam = 0 and s = x_H (when want_s).  Phase 1 stops at hare position 3H: if mu + lam <= H it detects the
// period by then (the tortoise sits at 2^k - 1 and detection comes at the first 2^k >= max(lam, mu + 1), so the
// hare is at 2^k - 1 + lam <= 3H - 2); phase 2 stops as soon as mu + lam would pass H.
template <typename T, typename P, bool kStaged, int MAXN>
__device__ __forceinline__ bool find_cycle(const DevArgs& a, const View<T, P, kStaged>& v, const int* x0, int& mu,
                                           int& lam, int* s, bool want_s) {
    const int N = a.N, H = a.H;
    int tort[MAXN], hare[MAXN];
    copy_rows<MAXN>(tort, x0, N);
    copy_rows<MAXN>(hare, x0, N);
    greedy_map<T, P, kStaged, MAXN>(a, v, hare);
    int power = 1, l = 1, pos = 1;
    bool det = false;
    for (;;) {
        if (same_rows<MAXN>(tort, hare, N)) { det = true; break; }
        if (pos >= 3 * H) break;
        if (power == l) { copy_rows<MAXN>(tort, hare, N); power <<= 1; l = 0; }
        greedy_map<T, P, kStaged, MAXN>(a, v, hare);
        l++;
        pos++;
    }
    bool found = det && l <= H;
    int m = 0;
    if (found) {
        copy_rows<MAXN>(tort, x0, N);
        copy_rows<MAXN>(hare, x0, N);
        for (int j = 0; j < l; j++) greedy_map<T, P, kStaged, MAXN>(a, v, hare);
        while (!same_rows<MAXN>(tort, hare, N)) {
            if (m + l >= H) { found = false; break; }
            greedy_map<T, P, kStaged, MAXN>(a, v, tort);
            greedy_map<T, P, kStaged, MAXN>(a, v, hare);
            m++;
        }
    }
    if (found) {
        mu = m;
        lam = l;
        copy_rows<MAXN>(s, tort, N);
    } else {
        mu = H;
        lam = 0;
        if (want_s) {
            copy_rows<MAXN>(s, x0, N);
            for (int j = 0; j < H; j++) greedy_map<T, P, kStaged, MAXN>(a, v, s);
        }
    }
    return found;
}

template <typename T, typename P, bool kStaged, int MAXN>
__global__ void __launch_bounds__(kDevTile) k_deviation(const DevArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    const int tid = threadIdx.x;
    const int G = a.G, N = a.N;
    const int64_t g0 = (int64_t)blockIdx.x * kDevTile;
    const int64_t g = g0 + tid;
    const T* __restrict__ qbase = reinterpret_cast<const T*>(a.q);
    double* lut = reinterpret_cast<double*>(s_mem);
    P* pol = reinterpret_cast<P*>(s_mem + ((a.lut_n * 8 + 15) & ~15));
    if constexpr (kStaged) {
        for (int j = tid; j < a.lut_n; j += kDevTile) {
            int i = 0;
            while (i + 1 < N && j >= a.lut_off[i + 1]) i++;
            lut[j] = scale_action(j - a.lut_off[i], a.ag[i]);
        }
        // entry e of local game gl at item gl * E + e: consecutive lanes take consecutive rows of one game
        const int E = a.pol_entries;
        const int n_loc = (int)(G - g0 < kDevTile ? G - g0 : kDevTile);
        for (int it = tid; it < n_loc * E; it += kDevTile) {
            const int gl = it / E, e = it - gl * E;
            int i = 0;
            while (i + 1 < N && e >= a.pol_off[i + 1]) i++;
            const AgentParams& p = a.ag[i];
            const int k = e - a.pol_off[i];
            const int row = k < a.win_n[i] ? a.win_lo[i] + k : encode64_fast(a.state0[g0 + gl], p);
            const T* qr = qbase + (g0 + gl) * a.stride + p.table_off + (int64_t)row * p.n_actions;
            pol[e * kDevTile + gl] = (P)argmax_row(qr, p.n_actions);
        }
        __syncthreads();
    }
    if (g >= G) return;
    View<T, P, kStaged> v{qbase + g * a.stride, pol + tid, lut};

    // pre-shock cycle
    int x0[MAXN], s[MAXN];
    const double st = a.state0[g];
#pragma unroll
    for (int i = 0; i < MAXN; i++)
        if (i < N) x0[i] = encode64_fast(st, a.ag[i]);
    int mu, lam;
    find_cycle<T, P, kStaged, MAXN>(a, v, x0, mu, lam, s, true);
    double cr[MAXN], ca[MAXN];
#pragma unroll
    for (int i = 0; i < MAXN; i++) { cr[i] = 0.0; ca[i] = 0.0; }
    if (lam > 0) {
        int x[MAXN], act[MAXN];
        double sc[MAXN], rew[MAXN];
        copy_rows<MAXN>(x, s, N);
        for (int j = 0; j < lam; j++) {
            greedy_actions<T, P, kStaged, MAXN>(a, v, x, act);
            transition<T, P, kStaged, MAXN>(a, v, act, sc, rew, x);
#pragma unroll
            for (int i = 0; i < MAXN; i++)
                if (i < N) { cr[i] = __dadd_rn(cr[i], rew[i]); ca[i] = __dadd_rn(ca[i], sc[i]); }
        }
#pragma unroll
        for (int i = 0; i < MAXN; i++)
            if (i < N) { cr[i] = __ddiv_rn(cr[i], (double)lam); ca[i] = __ddiv_rn(ca[i], (double)lam); }
    }

    // deviation path y and baseline path z, in lockstep
    const int d = a.d, L = a.L, K = a.K;
    const AgentParams& pd = a.ag[d];
    const double gam = a.sweep_gamma ? a.sweep_gamma[(int64_t)d * G + g] : pd.gamma;
    int y[MAXN], z[MAXN], yL[MAXN];
    copy_rows<MAXN>(y, s, N);
    copy_rows<MAXN>(z, s, N);
    copy_rows<MAXN>(yL, s, N);
    double gain = 0.0, w = 1.0;
    int adev = 0;
    const int64_t plane = (int64_t)N * G;
    for (int t = 0; t < K; t++) {
        int act[MAXN];
        double sc[MAXN], ry[MAXN];
        greedy_actions<T, P, kStaged, MAXN>(a, v, y, act);
        if (t < L) {
            int ad = a.dev_action;
            if (ad < 0) {           // one-period best response: argmax of d's reward, the others greedy (first max)
#pragma unroll
                for (int i = 0; i < MAXN; i++)
                    if (i < N) sc[i] = scaled_of(a, v, i, act[i]);
                double bv = 0.0;
                ad = 0;
                for (int k = 0; k < pd.n_actions; k++) {
                    const double sk = scaled_of(a, v, d, k);
#pragma unroll
                    for (int i = 0; i < MAXN; i++)
                        if (i < N && i == d) sc[i] = sk;
                    double rew[MAXN];
                    env_step<MAXN>(a.env, N, sc, a.env.a, rew);
                    const double r = pick<MAXN>(rew, d, N);
                    if (k == 0 || r > bv) { bv = r; ad = k; }
                }
            }
#pragma unroll
            for (int i = 0; i < MAXN; i++)
                if (i < N && i == d) act[i] = ad;
            if (t == 0) adev = ad;
        }
        transition<T, P, kStaged, MAXN>(a, v, act, sc, ry, y);
        const int rr = t - a.row_begin;
        if (rr >= 0 && rr < a.row_count) {
#pragma unroll
            for (int i = 0; i < MAXN; i++) {
                if (i >= N) break;
                const int64_t o = (int64_t)rr * plane + (int64_t)i * G + g;
                if (a.reward_rows) a.reward_rows[o] = ry[i];
                if (a.action_rows) a.action_rows[o] = sc[i];
            }
        }
        int actz[MAXN];
        double scz[MAXN], rz[MAXN];
        greedy_actions<T, P, kStaged, MAXN>(a, v, z, actz);
        transition<T, P, kStaged, MAXN>(a, v, actz, scz, rz, z);
        gain = __dadd_rn(gain, __dmul_rn(w, __dsub_rn(pick<MAXN>(ry, d, N), pick<MAXN>(rz, d, N))));
        w = __dmul_rn(w, gam);
        if (t + 1 == L) copy_rows<MAXN>(yL, y, N);
    }

    // return to the pre-shock cycle
    int mp, lp, sp[MAXN];
    const bool fp = find_cycle<T, P, kStaged, MAXN>(a, v, yL, mp, lp, sp, false);
    int ret = -1;
    if (lam > 0 && fp) {
        for (int j = 0; j < lp; j++) {
            if (same_rows<MAXN>(sp, s, N)) { ret = L + mp; break; }
            greedy_map<T, P, kStaged, MAXN>(a, v, sp);
        }
    }

    a.mu[g] = mu;
    a.lam[g] = lam;
    a.mu_post[g] = mp;
    a.lam_post[g] = lp;
    a.ret_step[g] = ret;
    a.act_dev[g] = adev;
    a.gain[g] = gain;
#pragma unroll
    for (int i = 0; i < MAXN; i++) {
        if (i >= N) break;
        a.cycle_reward[(int64_t)i * G + g] = cr[i];
        a.cycle_action[(int64_t)i * G + g] = ca[i];
    }
}

template <typename T, typename P, bool kStaged>
void launch_n(const DevArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.G + kDevTile - 1) / kDevTile)), block(kDevTile);
    const size_t lds = kStaged ? (size_t)a.lds_bytes : 0;
    if (a.N <= 2) hipLaunchKernelGGL((k_deviation<T, P, kStaged, 2>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((k_deviation<T, P, kStaged, THRL_MAXA>), grid, block, lds, s, a);
}

template <typename T>
void launch_t(const DevArgs& a, hipStream_t s) {
    if (!a.staged) launch_n<T, uint8_t, false>(a, s);
    else if (a.pol_bytes == 1) launch_n<T, uint8_t, true>(a, s);
    else launch_n<T, uint16_t, true>(a, s);
}

}  // namespace

int launch_deviation(const DevArgs& a, int q_dtype, hipStream_t s) {
    if (q_dtype == 1) launch_t<double>(a, s);
    else launch_t<float>(a, s);
    return (int)hipGetLastError();
}

}  // namespace thrl
