// thrl_converge.hip -- convergence tracking of the greedy policies (thrl_policy_track, include/thrl.h).
//
// A streaming pass bound by HBM reads: each game's tables are one contiguous block of stride elements.  One
// wavefront per block; block b takes games b, b + gridDim.x, ...  and counts the games that converge, with one
// atomic add on n_converged at the end.  Per game:
//   staged path: the game's block is copied into LDS with 16-byte loads, a batch of kUnroll in flight per lane (the
//     16-byte-aligned window around the block; the array's last partial chunk element by element, so nothing past
//     the first G games is read); the stored policy entries and the per-game words are requested before the batch,
//     so their latency overlaps it; then one row per lane, argmax from LDS;
//   direct path (a block larger than kTrackLdsBudget, or q not 16-byte aligned): one row per lane, argmax from HBM.
// The lanes compare their entries with the stored policy and write only those that differ (all of them for the
// baseline); a ballot tells whether the game changed; lane 0 writes the per-game words.  A game that converges is
// copied to q_conv from the same source (LDS or HBM), element by element: that write is paid once per game.
#include "thrl_converge.h"

namespace thrl {

namespace {

// 16-byte chunks per lane and batch: one batch covers the headline block (1,061 chunks in float32, 2,121 in float64)
template <typename T> constexpr int kUnroll = sizeof(T) == 4 ? 17 : 34;
constexpr int kPolPre = 4;              // stored policy entries per lane requested up front (P <= 256 in one go)

template <typename T, bool kStaged>
__global__ void __launch_bounds__(64) k_policy_track(const TrackArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    constexpr int kVec = 16 / sizeof(T);                 // elements per 16-byte chunk
    const int lane = threadIdx.x;
    const T* __restrict__ q = reinterpret_cast<const T*>(a.q);
    T* lds = reinterpret_cast<T*>(s_mem);
    const int64_t bound = (int64_t)a.G * a.stride;       // elements of the first G games
    int32_t n_conv = 0;
    for (int64_t g = blockIdx.x; g < a.G; g += gridDim.x) {
        const int64_t e0 = g * a.stride;
        uint16_t* pol = a.policy + g * a.P;
        uint16_t old[kPolPre];
        int64_t since = 0, conv = 0;
        if (!a.baseline) {
#pragma unroll
            for (int k = 0; k < kPolPre; k++) {
                const int r = lane + 64 * k;
                old[k] = r < a.P ? pol[r] : 0;
            }
            since = a.stable_since[g];
            conv = a.converged_at[g];
        }
        const T* src;
        if constexpr (kStaged) {
            const int64_t w0 = e0 & ~(int64_t)(kVec - 1);
            const int64_t w1 = (e0 + a.stride + kVec - 1) & ~(int64_t)(kVec - 1);
            const int64_t wend = w1 < bound ? w1 : bound;
            const int nfull = (int)((wend - w0) / kVec);     // whole chunks inside [0, bound)
            const uint4* g4 = reinterpret_cast<const uint4*>(q + w0);
            uint4* l4 = reinterpret_cast<uint4*>(s_mem);
            // Lanes past the end load the last chunk and store it back to its own place: no branch around the
            // stores, so the compiler keeps the whole batch of loads in flight before the first LDS write.
            for (int c0 = 0; c0 < nfull; c0 += kUnroll<T> * 64) {
                uint4 v[kUnroll<T>];
#pragma unroll
                for (int u = 0; u < kUnroll<T>; u++) {
                    const int c = c0 + u * 64 + lane;
                    v[u] = g4[c < nfull ? c : nfull - 1];
                }
#pragma unroll
                for (int u = 0; u < kUnroll<T>; u++) {
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

        bool changed = false;
        for (int r = lane, k = 0; r < a.P; r += 64, k++) {
            int i = 0;
            while (i + 1 < a.N && r >= a.row_off[i + 1]) i++;
            const int na = a.n_actions[i];
            const uint16_t act = (uint16_t)argmax_row(src + a.table_off[i] + (int64_t)(r - a.row_off[i]) * na, na);
            if (a.baseline) {
                pol[r] = act;
            } else {
                uint16_t prev = k < kPolPre ? 0 : pol[r];
#pragma unroll
                for (int j = 0; j < kPolPre; j++)
                    if (j == k) prev = old[j];
                if (act != prev) {
                    pol[r] = act;
                    changed = true;
                }
            }
        }
        const bool any = __ballot(changed) != 0;

        if (a.baseline) {
            if (lane == 0) {
                a.stable_since[g] = a.episode;
                a.converged_at[g] = -1;
                a.conv_since[g] = -1;
                a.changes[g] = 0;
            }
        } else {
            if (any) {
                since = a.episode;
                if (lane == 0) {
                    a.stable_since[g] = since;
                    a.changes[g] = a.changes[g] + 1;
                }
            }
            if (conv < 0 && a.episode - since >= a.window) {
                n_conv++;
                if (lane == 0) {
                    a.converged_at[g] = a.episode;
                    a.conv_since[g] = since;
                    if (a.q_conv) a.state_conv[g] = a.state[g];
                }
                if (a.q_conv) {
                    T* dst = reinterpret_cast<T*>(a.q_conv) + e0;
                    for (int64_t k = lane; k < a.stride; k += 64) dst[k] = src[k];
                }
            }
        }
        if constexpr (kStaged) __syncthreads();          // this game's LDS reads before the next game's writes
    }
    if (lane == 0 && n_conv && a.n_converged) atomicAdd(a.n_converged, n_conv);
}

template <typename T>
void launch_t(const TrackArgs& a, int grid, hipStream_t s) {
    if (a.staged)
        hipLaunchKernelGGL((k_policy_track<T, true>), dim3(grid), dim3(64), (size_t)a.lds_bytes, s, a);
    else
        hipLaunchKernelGGL((k_policy_track<T, false>), dim3(grid), dim3(64), 0, s, a);
}

}  // namespace

int launch_policy_track(const TrackArgs& a, int q_dtype, int grid, hipStream_t s) {
    if (q_dtype == 1) launch_t<double>(a, grid, s);
    else launch_t<float>(a, grid, s);
    return (int)hipGetLastError();
}

}  // namespace thrl
