// thrl_stats.hip -- per-group histogram, fixed-point moments and exact min / max of per-game episode rows
// (thrl_group_stats, include/thrl.h).  Integer-only accumulation, so the result does not depend on the launch
// geometry, the order of the atomics, the cut of the episodes into calls or of the games into shards.
#include <math.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "../../include/thrl.h"

namespace thrl {

namespace {

constexpr int kStatsBlock = 256;          // 4 waves
constexpr int kStatsWaves = kStatsBlock / 64;
constexpr int kStatsPeel = 2;             // bins taken whole by a ballot before the remaining lanes add one by one

struct StatsArgs {
    int32_t G, N, E, n_groups, B, Q;
    int64_t tile;                         // games (positions of perm) per block
    const double* rew;
    const double* act;
    const int32_t* perm;
    const int64_t* seg_off;
    double lo[THRL_STATS_MAXQ], hi[THRL_STATS_MAXQ], inv_w[THRL_STATS_MAXQ], M[THRL_STATS_MAXQ];
    double s1[THRL_STATS_MAXQ], s2[THRL_STATS_MAXQ];
    uint32_t* hist;
    int64_t* sums;
    uint64_t* minmax;
};

__device__ __forceinline__ uint64_t order_key(double x) {
    const uint64_t u = (uint64_t)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ int64_t clamp_seg(int64_t v, int64_t G) { return v < 0 ? 0 : (v > G ? G : v); }

// One block: for each (episode, quantity) pair of its y-stride, the positions [t0, t1) of perm, cut at group
// boundaries; per piece an LDS histogram, then one global atomic per non-zero bin and one per moment / extreme.
__global__ void __launch_bounds__(kStatsBlock) k_group_stats(const StatsArgs a) {
    __shared__ uint32_t s_hist[THRL_STATS_MAX_BINS + 2];
    __shared__ unsigned long long s_sum[2];
    __shared__ unsigned long long s_key[2];
    __shared__ int s_first;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int nb = a.B + 2;
    const int64_t G = a.G;
    const int64_t t0 = (int64_t)blockIdx.x * a.tile;
    if (t0 >= G) return;
    const int64_t t1 = t0 + a.tile < G ? t0 + a.tile : G;
    // first group whose segment ends after t0 (seg_off is non-decreasing for a valid spec; clamped for safety)
    if (tid == 0) {
        int lo = 0, hi = a.n_groups;              // answer in [0, n_groups]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (clamp_seg(a.seg_off[mid + 1], G) > t0) hi = mid; else lo = mid + 1;
        }
        s_first = lo;
    }
    for (int j = tid; j < nb; j += kStatsBlock) s_hist[j] = 0u;
    if (tid < 2) { s_sum[tid] = 0ull; s_key[tid] = 0ull; }
    __syncthreads();
    const int first = s_first;
    const int64_t plane = (int64_t)a.N * G;
    for (int pair = blockIdx.y; pair < a.E * a.Q; pair += gridDim.y) {
        const int e = pair / a.Q, q = pair - e * a.Q;
        const double lo = a.lo[q], hi = a.hi[q], inv_w = a.inv_w[q], M = a.M[q], s1 = a.s1[q], s2 = a.s2[q];
        const double* row = q < a.N ? a.rew + e * plane + (int64_t)q * G
                                    : (q < 2 * a.N ? a.act + e * plane + (int64_t)(q - a.N) * G : a.rew + e * plane);
        const bool total = q == 2 * a.N;
        for (int k = first; k < a.n_groups; k++) {
            const int64_t g0 = clamp_seg(a.seg_off[k], G), g1 = clamp_seg(a.seg_off[k + 1], G);
            if (g0 >= t1) break;
            const int64_t p0 = g0 > t0 ? g0 : t0, p1 = g1 < t1 ? g1 : t1;
            if (p1 <= p0) continue;                                   // block-uniform
            long long m1 = 0, m2 = 0;
            uint64_t kmin = 0, kmax = 0;                              // ~key(min) and key(max); 0 = none
            // whole waves run the loop so the ballots see every lane; lanes past p1 take no bin
            for (int64_t base = p0; base < p1; base += kStatsBlock) {
                const int64_t p = base + tid;
                int bin = -1;
                if (p < p1) {
                    const int32_t g = a.perm[p];
                    if (g >= 0 && (int64_t)g < G) {
                        double x;
                        if (total) {
                            x = row[g];
                            for (int i = 1; i < a.N; i++) x = x + row[(int64_t)i * G + g];
                        } else {
                            x = row[g];
                        }
                        if (!isfinite(x)) {
                            bin = a.B + 1;
                        } else {
                            if (x < lo) bin = 0;
                            else if (x >= hi) bin = a.B + 1;
                            else {
                                const int b = (int)floor((x - lo) * inv_w);
                                bin = 1 + (b < a.B - 1 ? b : a.B - 1);
                            }
                            const double xc = x < -M ? -M : (x > M ? M : x);
                            m1 += (long long)rint(xc * s1);
                            m2 += (long long)rint((xc * xc) * s2);
                            const uint64_t kx = order_key(x);
                            kmin = (~kx > kmin) ? ~kx : kmin;
                            kmax = kx > kmax ? kx : kmax;
                        }
                    }
                }
                // wave aggregation: the bins of the first active lanes are taken whole (a converged group's
                // games share a handful of bins), then each remaining lane adds its own
                bool pending = bin >= 0;
#pragma unroll
                for (int r = 0; r < kStatsPeel; r++) {
                    const unsigned long long act = __ballot(pending);
                    if (act == 0ull) break;
                    const int leader = __ffsll((long long)act) - 1;
                    const int lb = __shfl(bin, leader);
                    const unsigned long long same = __ballot(pending && bin == lb);
                    if (lane == leader) atomicAdd(&s_hist[lb], (uint32_t)__popcll(same));
                    if (pending && bin == lb) pending = false;
                }
                if (pending) atomicAdd(&s_hist[bin], 1u);
            }
            // moments and extremes: wave reduction, then one LDS atomic per wave
            for (int off = 32; off > 0; off >>= 1) {
                m1 += __shfl_down(m1, off);
                m2 += __shfl_down(m2, off);
                const uint64_t o0 = (uint64_t)__shfl_down((long long)kmin, off);
                const uint64_t o1 = (uint64_t)__shfl_down((long long)kmax, off);
                kmin = o0 > kmin ? o0 : kmin;
                kmax = o1 > kmax ? o1 : kmax;
            }
            if (lane == 0) {
                atomicAdd(&s_sum[0], (unsigned long long)m1);
                atomicAdd(&s_sum[1], (unsigned long long)m2);
                atomicMax(&s_key[0], (unsigned long long)kmin);
                atomicMax(&s_key[1], (unsigned long long)kmax);
            }
            __syncthreads();
            const int64_t cell = ((int64_t)e * a.n_groups + k) * a.Q + q;
            uint32_t* gh = a.hist + cell * nb;
            for (int j = tid; j < nb; j += kStatsBlock) {
                const uint32_t c = s_hist[j];
                if (c) { atomicAdd(gh + j, c); s_hist[j] = 0u; }
            }
            if (tid == 0) {
                atomicAdd((unsigned long long*)(a.sums + cell * 2), s_sum[0]);
                atomicAdd((unsigned long long*)(a.sums + cell * 2 + 1), s_sum[1]);
                if (s_key[0]) atomicMax((unsigned long long*)(a.minmax + cell * 2), s_key[0]);
                if (s_key[1]) atomicMax((unsigned long long*)(a.minmax + cell * 2 + 1), s_key[1]);
                s_sum[0] = s_sum[1] = 0ull;
                s_key[0] = s_key[1] = 0ull;
            }
            __syncthreads();
        }
    }
}

}  // namespace

// Launch for an args block thrl_group_stats (thrl_api_analysis.hip) has validated.  Geometry: tiles of perm positions
// on x, (episode, quantity) pairs on y, sized so the grid holds a few thousand blocks; results do not depend on it.
int launch_group_stats(const thrl_group_stats_args* g, hipStream_t s) {
    StatsArgs a;
    memset(&a, 0, sizeof(a));
    a.G = g->n_games; a.N = g->n_agents; a.E = g->n_episodes; a.n_groups = g->n_groups; a.B = g->n_bins;
    a.Q = 2 * g->n_agents + 1;
    a.rew = g->game_reward_log; a.act = g->game_action_log; a.perm = g->perm; a.seg_off = g->seg_off;
    for (int q = 0; q < a.Q; q++) {
        a.lo[q] = g->lo[q]; a.hi[q] = g->hi[q]; a.inv_w[q] = g->inv_w[q];
        a.M[q] = 16.0 * fmax(fabs(g->lo[q]), fabs(g->hi[q]));
        a.s1[q] = g->scale[q][0]; a.s2[q] = g->scale[q][1];
    }
    a.hist = g->hist; a.sums = g->sums; a.minmax = g->minmax;
    const int64_t pairs = (int64_t)a.E * a.Q;
    const int64_t gy = pairs < 65535 ? pairs : 65535;
    const int64_t target = 4096;
    int64_t tx = target / gy;
    if (tx < 1) tx = 1;
    int64_t tile = ((int64_t)a.G + tx - 1) / tx;
    const int64_t min_tile = 4 * kStatsBlock;
    if (tile < min_tile) tile = min_tile;
    tile = (tile + kStatsBlock - 1) / kStatsBlock * kStatsBlock;
    a.tile = tile;
    const int64_t gx = ((int64_t)a.G + tile - 1) / tile;
    hipLaunchKernelGGL(k_group_stats, dim3((unsigned)gx, (unsigned)gy), dim3(kStatsBlock), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace thrl
