// response_check.h -- what tests/sampled_response_check.cpp and tests/sampled_response_noise_check.cpp share: the shims
// under which a response kernel's source compiles for the host (include this, then the kernel's .hip), the reader and the
// bit-for-bit comparison of their case files, and the runner of a block as host threads with barriers.
#pragma once
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

// the shared solver pieces first, as HIP declares them: improve_margin, first_max, rel_loss and the band's limits are
// __host__ __device__
#include "../th_rl_amd/csrc/thrl_solve_dev.h"

// from here on a __device__ function is a host function, a barrier is the host threads', an _rn operation a plain one
// (the build's -ffp-contract=off rounds each separately)
static std::barrier<>* g_bar;
#undef __device__
#define __device__
#define __syncthreads() g_bar->arrive_and_wait()
#define __dadd_rn(a, b) ((a) + (b))
#define __dsub_rn(a, b) ((a) - (b))
#define __dmul_rn(a, b) ((a) * (b))
#define __ddiv_rn(a, b) ((a) / (b))

template <typename T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}

template <typename T>
static int cmp(const char* what, const std::vector<T>& a, const std::vector<T>& b) {
    int bad = 0;
    for (size_t i = 0; i < a.size(); i++) bad += memcmp(&a[i], &b[i], sizeof(T)) != 0;
    if (bad) printf("  %s: %d of %zu differ\n", what, bad, a.size());
    return bad;
}

// nblk blocks in turn, each as `threads` host threads that meet at g_bar: thread(mem, t, b) is thread t of block b on
// the block's working set mem
template <typename F>
static void run_blocks(long long lds, int nblk, int threads, F thread) {
    for (int b = 0; b < nblk; b++) {
        // exactly lds bytes, on the heap: an access past the working set is an access past the allocation
        unsigned char* mem = static_cast<unsigned char*>(aligned_alloc(16, (size_t)lds));
        std::barrier<> bar(threads);
        g_bar = &bar;
        std::vector<std::thread> th;
        for (int t = 0; t < threads; t++) th.emplace_back([&, t] { thread(mem, t, b); });
        for (auto& x : th) x.join();
        free(mem);
    }
}
