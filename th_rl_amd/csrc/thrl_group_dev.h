// thrl_group_dev.h -- the stable grouping the chain kernels on action tuples share word for word: k_ts_chain
// (thrl_tuple_stationary.hip) and k_tdn_chain (thrl_tuple_deviation_noise.hip).  Both turn "sum the masses of the items
// that map to tuple t'" into a segmented sum in ascending index order: the items are sorted once per game by the tuple
// their strategy entries name.  A device inline function only, in namespace thrl's anonymous namespace, once per
// including file.  It contains barriers: every thread of the block calls it.
#pragma once
#include <stdint.h>

namespace thrl {

namespace {

// the stable grouping of n items by key(idx) in [0, T): perm[s] = the idx at sorted place s, first[key] = the first place
// with a key >= key (first[T] = n), so the items of key are perm[first[key] .. first[key + 1]).  key(idx) is the tuple of
// the clamped entries pol[i][src], src = idx, or with a map src = map[idx] (the item is looked up where the map sends
// it).  A bitonic sort of the 32-bit words (key << 16 | idx) in srt, whose order IS the stable one since the words are
// distinct; srt holds the next power of two >= n words.  Args: N, T, n_actions[], tstride[].
template <int kBlock, typename Args>
__device__ __forceinline__ void ts_group(const Args& a, const uint16_t* __restrict__ pol, const uint16_t* map, int n,
                                         uint32_t* srt, uint16_t* perm, uint16_t* first, int tid) {
    int p2 = 1;
    while (p2 < n) p2 <<= 1;
    __syncthreads();                                     // whatever read the aliased arrays is done
    for (int idx = tid; idx < p2; idx += kBlock) {
        uint32_t w = 0xffffffffu;
        if (idx < n) {
            const int src = map ? (int)map[idx] : idx;
            int key = 0;
            for (int i = 0; i < a.N; i++) key += min((int)pol[(int64_t)i * n + src], a.n_actions[i] - 1) * a.tstride[i];
            w = ((uint32_t)key << 16) | (uint32_t)idx;
        }
        srt[idx] = w;
    }
    __syncthreads();
    for (int k = 2; k <= p2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int idx = tid; idx < p2; idx += kBlock) {
                const int ixj = idx ^ j;
                if (ixj > idx) {
                    const uint32_t x = srt[idx], y = srt[ixj];
                    if ((x > y) == ((idx & k) == 0)) { srt[idx] = y; srt[ixj] = x; }
                }
            }
            __syncthreads();
        }
    }
    for (int s = tid; s < n; s += kBlock) {
        const uint32_t w = srt[s];
        const int key = (int)(w >> 16);
        perm[s] = (uint16_t)(w & 0xffffu);
        const int prev = s > 0 ? (int)(srt[s - 1] >> 16) : -1;
        for (int kk = prev + 1; kk <= key; kk++) first[kk] = (uint16_t)s;
        if (s == n - 1)
            for (int kk = key + 1; kk <= a.T; kk++) first[kk] = (uint16_t)n;
    }
    __syncthreads();
}

}  // namespace

}  // namespace thrl
