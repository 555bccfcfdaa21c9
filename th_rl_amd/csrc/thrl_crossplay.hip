// thrl_crossplay.hip -- cross-play of the greedy policies (thrl_crossplay, include/thrl.h): agent i of one game seated
// against the agents of other games, and the limit cycle of their greedy play.  Two kernels.
//
// k_xplay_extract: the greedy policy of every game, 2 bytes per table row.  A streaming pass bound by HBM reads, the
//   memory pattern of the convergence tracker's baseline pass: one wavefront per block, block b takes
//   games b, b + gridDim.x, ...; the game's contiguous block is copied into LDS with 16-byte loads, a whole batch in
//   flight per lane before the first LDS write, then one row per lane, argmax from LDS.  Blocks larger than
//   kXpExtractLdsBudget, or a q that is not 16-byte aligned, take the direct path: one row per lane from HBM.
//
// k_xplay_walk: one lane per match.  A match only ever reads, of each seat's policy, the window of rows the action
//   grids can produce plus x_0's row.  Staged path: the block copies those entries of its matches into
//   LDS (consecutive lanes take consecutive entries of one game's window, so the gather is a run of 2-byte loads per
//   seat) together with a LUT of every agent's scaled actions; the walk then touches no global memory.  Configs whose
//   windows do not fit kXpLdsBudget gather each visited entry from the policy array.  Both paths walk the same map with
//   the same operations, so both give the same bits.  The cycle search, the refused match's zeros, the store of the
//   means and of the row slice, the window lookup and the LUT fill are thrl_walk_dev.h's.
#include "thrl_crossplay.h"

#include "thrl_walk_dev.h"

namespace thrl {

namespace {

// ------------------------------------------------------------------------------------------------ extraction
// 16-byte chunks per lane and batch: one batch covers the headline block (1,061 chunks in float32, 2,121 in float64)
template <typename T> constexpr int kXpUnroll = sizeof(T) == 4 ? 17 : 34;

template <typename T, bool kStaged>
__global__ void __launch_bounds__(64) k_xplay_extract(const XpExtractArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    constexpr int kVec = 16 / sizeof(T);                 // elements per 16-byte chunk
    const int lane = threadIdx.x;
    const T* __restrict__ q = reinterpret_cast<const T*>(a.q);
    T* lds = reinterpret_cast<T*>(s_mem);
    const int64_t bound = (int64_t)a.G * a.stride;       // elements of the first G games
    for (int64_t g = blockIdx.x; g < a.G; g += gridDim.x) {
        const int64_t e0 = g * a.stride;
        uint16_t* pol = a.policy + g * a.P;
        const T* src;
        if constexpr (kStaged) {
            // the 16-byte-aligned window around the block; the array's last partial chunk element by element, so
            // nothing past the first G games is read
            const int64_t w0 = e0 & ~(int64_t)(kVec - 1);
            const int64_t w1 = (e0 + a.stride + kVec - 1) & ~(int64_t)(kVec - 1);
            const int64_t wend = w1 < bound ? w1 : bound;
            const int nfull = (int)((wend - w0) / kVec);
            const uint4* g4 = reinterpret_cast<const uint4*>(q + w0);
            uint4* l4 = reinterpret_cast<uint4*>(s_mem);
            // Lanes past the end load the last chunk and store it back to its own place: no branch around the
            // stores, so the loads of a batch can be in flight together.  (hipcc still pairs the first few loads with
            // their LDS writes here, which k_policy_track's schedule does not; a scheduling barrier between the two
            // loops was measured and is worse: DESIGN 5.11.)
            for (int c0 = 0; c0 < nfull; c0 += kXpUnroll<T> * 64) {
                uint4 v[kXpUnroll<T>];
#pragma unroll
                for (int u = 0; u < kXpUnroll<T>; u++) {
                    const int c = c0 + u * 64 + lane;
                    v[u] = g4[c < nfull ? c : nfull - 1];
                }
#pragma unroll
                for (int u = 0; u < kXpUnroll<T>; u++) {
                    const int c = c0 + u * 64 + lane;
                    l4[c < nfull ? c : nfull - 1] = v[u];
                }
            }
            for (int64_t e = w0 + (int64_t)nfull * kVec + lane; e < wend; e += 64) lds[e - w0] = q[e];
            __syncthreads();
            src = lds + (e0 - w0);
        } else {
            src = q + e0;
        }
        for (int r = lane; r < a.P; r += 64) {
            int i = 0;
            while (i + 1 < a.N && r >= a.row_off[i + 1]) i++;
            const int na = a.n_actions[i];
            pol[r] = (uint16_t)argmax_row(src + a.table_off[i] + (int64_t)(r - a.row_off[i]) * na, na);
        }
        if constexpr (kStaged) __syncthreads();          // this game's LDS reads before the next game's writes
    }
}

template <typename T>
void launch_extract_t(const XpExtractArgs& a, int grid, hipStream_t s) {
    if (a.staged)
        hipLaunchKernelGGL((k_xplay_extract<T, true>), dim3(grid), dim3(64), (size_t)a.lds_bytes, s, a);
    else
        hipLaunchKernelGGL((k_xplay_extract<T, false>), dim3(grid), dim3(64), 0, s, a);
}

// ------------------------------------------------------------------------------------------------ walk
template <bool kStaged, int MAXN>
struct Seats {                      // where a lane finds the greedy policies of its match
    const uint16_t* pol;            // staged: entry e of this lane's match at pol[e * kXpTile]
    const uint16_t* gp[MAXN];       // direct: agent i's rows of the seated game, gp[i][row]
    const double* lut;              // scaled actions (use_lut), agent i's at lut[lut_off[i] ..]
};

template <bool kStaged, int MAXN>
__device__ __forceinline__ int policy(const XpWalkArgs& a, const Seats<kStaged, MAXN>& v, int i, int r) {
    int act;
    if constexpr (kStaged) {
        act = (int)v.pol[window_entry(a, i, r) * kXpTile];
    } else {
        act = (int)v.gp[i][r];
    }
    return min(act, a.ag[i].n_actions - 1);
}

// One transition from x under the greedy policies: scaled actions, rewards, and the next rows into x.
template <bool kStaged, int MAXN>
__device__ __forceinline__ void step(const XpWalkArgs& a, const Seats<kStaged, MAXN>& v, double* sc, double* rew, int* x) {
    const int N = a.N;
#pragma unroll
    for (int i = 0; i < MAXN; i++)
        if (i < N) {
            const int act = policy<kStaged, MAXN>(a, v, i, x[i]);
            sc[i] = a.use_lut ? v.lut[a.lut_off[i] + act] : scale_action(act, a.ag[i]);
        }
    const double p = env_step<MAXN>(a.env, N, sc, a.env.a, rew);
#pragma unroll
    for (int i = 0; i < MAXN; i++)
        if (i < N) x[i] = encode64_fast(p, a.ag[i]);
}

template <bool kStaged, int MAXN>
__global__ void __launch_bounds__(kXpTile) k_xplay_walk(const XpWalkArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    const int tid = threadIdx.x;
    const int M = a.M, N = a.N;
    const int64_t m0 = (int64_t)blockIdx.x * kXpTile;
    const int64_t m = m0 + tid;
    double* lut = reinterpret_cast<double*>(s_mem);
    uint16_t* pol = reinterpret_cast<uint16_t*>(s_mem + (a.use_lut ? ((a.lut_n * 8 + 15) & ~15) : 0));
    if (a.use_lut) fill_scale_lut(a, lut, tid, kXpTile);
    if constexpr (kStaged) {
        // entry e of local match ml at item ml * E + e: consecutive lanes take consecutive rows of one seat's window
        const int E = a.pol_entries;
        const int n_loc = (int)(M - m0 < kXpTile ? M - m0 : kXpTile);
        for (int it = tid; it < n_loc * E; it += kXpTile) {
            const int ml = it / E, e = it - ml * E;
            const int i = window_agent(a, e);
            const int64_t g = a.seat[(int64_t)i * M + m0 + ml];
            uint16_t act = 0;
            if (g >= 0 && g < a.G)                       // a seat out of range reads nothing
                act = a.policy[g * a.P + a.row_off[i] + window_row(a, i, e, a.state0[m0 + ml])];
            pol[e * kXpTile + ml] = act;
        }
    }
    if (a.use_lut || kStaged) __syncthreads();
    if (m >= M) return;

    Seats<kStaged, MAXN> v;
    v.pol = pol + tid;
    v.lut = lut;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < MAXN; i++) {
        if (i >= N) break;
        const int64_t g = a.seat[(int64_t)i * M + m];
        const bool in = g >= 0 && g < a.G;
        ok = ok && in;
        if constexpr (!kStaged) v.gp[i] = a.policy + (in ? g : 0) * a.P + a.row_off[i];
    }
    if (!ok) {                                          // the stated sentinel: mu = -1, lam = 0 and zeros
        a.mu[m] = -1;
        a.lam[m] = 0;
        store_refused(a, m, M);
        return;
    }

    int x0[MAXN], s[MAXN];
    const double st = a.state0[m];
#pragma unroll
    for (int i = 0; i < MAXN; i++)
        if (i < N) x0[i] = encode64_fast(st, a.ag[i]);
    int mu, lam;
    find_cycle(x0, N, a.H, [&](int* x) THRL_WALK_INLINE {               // x <- F(x): the greedy map on row tuples
        double sc[MAXN], rew[MAXN];
        step<kStaged, MAXN>(a, v, sc, rew, x);
    }, mu, lam, s, false);
    // cycle_means of thrl_walk_dev.h, kept inline: through the shared function <direct, 8> takes 196 VGPRs for 156 and
    // loses a wave per SIMD (profiles/walk_shared_resource_usage.txt)
    double cr[MAXN], ca[MAXN];
#pragma unroll
    for (int i = 0; i < MAXN; i++) { cr[i] = 0.0; ca[i] = 0.0; }
    if (lam > 0) {
        int x[MAXN];
        double sc[MAXN], rew[MAXN];
        copy_rows<MAXN>(x, s, N);
        for (int j = 0; j < lam; j++) {
            step<kStaged, MAXN>(a, v, sc, rew, x);
#pragma unroll
            for (int i = 0; i < MAXN; i++)
                if (i < N) { cr[i] = __dadd_rn(cr[i], rew[i]); ca[i] = __dadd_rn(ca[i], sc[i]); }
        }
#pragma unroll
        for (int i = 0; i < MAXN; i++)
            if (i < N) { cr[i] = __ddiv_rn(cr[i], (double)lam); ca[i] = __ddiv_rn(ca[i], (double)lam); }
    }
    a.mu[m] = mu;
    a.lam[m] = lam;
    store_means<MAXN>(a, m, M, cr, ca);

    // the path from x_0: the rows of tau in [row_begin, row_begin + row_count)
    if (a.row_count > 0 && (a.reward_rows || a.action_rows)) {
        int x[MAXN];
        double sc[MAXN], rew[MAXN];
        copy_rows<MAXN>(x, x0, N);
        const int end = a.row_begin + a.row_count;
        for (int t = 0; t < end; t++) {
            step<kStaged, MAXN>(a, v, sc, rew, x);
            store_step<MAXN>(a, t, m, M, StepOut{rew, sc, 1});
        }
    }
}

template <bool kStaged>
void launch_walk_n(const XpWalkArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)(((int64_t)a.M + kXpTile - 1) / kXpTile)), block(kXpTile);
    const size_t lds = (size_t)a.lds_bytes;
    if (a.N <= 2) hipLaunchKernelGGL((k_xplay_walk<kStaged, 2>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((k_xplay_walk<kStaged, THRL_MAXA>), grid, block, lds, s, a);
}

}  // namespace

int launch_xplay_extract(const XpExtractArgs& a, int q_dtype, int grid, hipStream_t s) {
    if (q_dtype == 1) launch_extract_t<double>(a, grid, s);
    else launch_extract_t<float>(a, grid, s);
    return (int)hipGetLastError();
}

int launch_xplay_walk(const XpWalkArgs& a, hipStream_t s) {
    if (a.staged) launch_walk_n<true>(a, s);
    else launch_walk_n<false>(a, s);
    return (int)hipGetLastError();
}

}  // namespace thrl
