// thrl_deviation.hip -- deviation analysis of the greedy policies (thrl_deviation, include/thrl.h): the limit
// cycle of greedy play, a forced deviation of one agent, the response of the others, the discounted gain of the
// deviator and whether play returns to the cycle.  One lane per game.
//
// Staged path: the block first stages every game's greedy policy into LDS -- the argmax of each row the walk can
// reach (the window of rows the action grids can produce, plus x_0's row), one byte or two per entry -- and a LUT
// of every agent's scaled actions.  The walk then needs no table reads and no division in scale_action.  Configs
// whose policy does not fit kDevLdsBudget take the direct path, which reads each visited row from HBM.  Both walk
// the same map with the same operations, so both give the same bits.  The cycle search, the means over the cycle, the
// store of the row slice, the window lookup and the LUT fill are thrl_walk_dev.h's; the map, the staging loop's argmax
// and the lockstep deviation / baseline loop are this file's.
#include "thrl_deviation.h"

#include "thrl_walk_dev.h"

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
        return (int)v.pol[window_entry(a, i, r) * kDevTile];
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
        fill_scale_lut(a, lut, tid, kDevTile);
        // entry e of local game gl at item gl * E + e: consecutive lanes take consecutive rows of one game
        const int E = a.pol_entries;
        const int n_loc = (int)(G - g0 < kDevTile ? G - g0 : kDevTile);
        for (int it = tid; it < n_loc * E; it += kDevTile) {
            const int gl = it / E, e = it - gl * E;
            const int i = window_agent(a, e);
            const AgentParams& p = a.ag[i];
            const int row = window_row(a, i, e, a.state0[g0 + gl]);
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
    const auto next = [&](int* x) THRL_WALK_INLINE { greedy_map<T, P, kStaged, MAXN>(a, v, x); };
    int mu, lam;
    find_cycle(x0, N, a.H, next, mu, lam, s, true);
    double cr[MAXN], ca[MAXN];
    {
        int x[MAXN], act[MAXN];
        double sc[MAXN], rew[MAXN];
        copy_rows<MAXN>(x, s, N);
        cycle_means<MAXN>(N, lam, cr, ca, [&]() THRL_WALK_INLINE {
            greedy_actions<T, P, kStaged, MAXN>(a, v, x, act);
            transition<T, P, kStaged, MAXN>(a, v, act, sc, rew, x);
            return StepOut{rew, sc, 1};
        });
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
        store_step<MAXN>(a, t, g, G, StepOut{ry, sc, 1});
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
    const bool fp = find_cycle(yL, N, a.H, next, mp, lp, sp, false);
    int ret = -1;
    if (lam > 0 && fp) {
        for (int j = 0; j < lp; j++) {
            if (same_rows<MAXN>(sp, s, N)) { ret = L + mp; break; }
            next(sp);
        }
    }

    a.mu[g] = mu;
    a.lam[g] = lam;
    a.mu_post[g] = mp;
    a.lam_post[g] = lp;
    a.ret_step[g] = ret;
    a.act_dev[g] = adev;
    a.gain[g] = gain;
    store_means<MAXN>(a, g, G, cr, ca);
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
