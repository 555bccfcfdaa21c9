// sampled_host_check.cpp -- k_sp_chain's source (th_rl_amd/csrc/thrl_sampled.hip) compiled for the host and run as 256
// threads with barriers, for address / undefined-behaviour sanitizers.  Reads the inputs and the mirror's outputs that
// profiles/sampled_host_check.py writes, runs every game through sp_block and compares every output bit for bit.
// Build and run: see profiles/sampled_host_check.py.  No GPU is involved.
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

static std::barrier<>* g_bar;
#define __device__
#define __forceinline__ inline
#define __syncthreads() g_bar->arrive_and_wait()
static inline double __dadd_rn(double a, double b) { return a + b; }
static inline double __dsub_rn(double a, double b) { return a - b; }
static inline double __dmul_rn(double a, double b) { return a * b; }
static inline double __ddiv_rn(double a, double b) { return a / b; }
using std::max;
using std::min;

#include "thrl_sampled.hip"

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

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    auto h = rd<int32_t>(f, 8);                          // G N T D max_iters start_tuple has_eps_g n_blocks
    thrl::SpArgs a;
    memset(&a, 0, sizeof(a));
    a.G = h[0]; a.N = h[1]; a.T = h[2]; a.D = h[3]; a.max_iters = h[4]; a.start_tuple = h[5];
    const int nblk = h[7];
    auto kind = rd<int32_t>(f, 8), nact = rd<int32_t>(f, 8);
    auto eps = rd<double>(f, 8), tol = rd<double>(f, 1);
    int ts = 1;
    for (int i = a.N - 1; i >= 0; i--) {
        a.kind[i] = kind[i]; a.n_actions[i] = nact[i]; a.tstride[i] = ts; ts *= nact[i]; a.eps[i] = eps[i];
    }
    a.tol = tol[0];
    const size_t G = a.G, N = a.N, T = a.T, D = a.D;
    auto eps_g = rd<double>(f, h[6] ? N * G : 0);
    auto start = rd<int32_t>(f, G);
    std::vector<std::vector<float>> prob(N);
    for (size_t i = 0; i < N; i++) prob[i] = rd<float>(f, kind[i] ? G * D * nact[i] : 0);
    auto dpol = rd<uint16_t>(f, G * N * D);
    auto first = rd<int32_t>(f, D + 1), perm = rd<int32_t>(f, T);
    auto reward = rd<double>(f, N * T), scaled = rd<double>(f, N * T), price = rd<double>(f, T);
    auto w_iters = rd<int32_t>(f, G);
    auto w_change = rd<double>(f, G), w_mass = rd<double>(f, G), w_rew = rd<double>(f, N * G), w_act = rd<double>(f, N * G),
         w_price = rd<double>(f, G), w_agree = rd<double>(f, G), w_pi = rd<double>(f, G * T);
    fclose(f);
    std::vector<int32_t> iters(G, -7);
    std::vector<double> change(G, -7), mass(G, -7), rew(N * G, -7), act(N * G, -7), sprice(G, -7), agree(G, -7), pi(G * T, -7);
    a.eps_g = h[6] ? eps_g.data() : nullptr; a.start = start.data(); a.dpolicy = dpol.data();
    for (size_t i = 0; i < N; i++) a.prob[i] = kind[i] ? prob[i].data() : nullptr;
    a.grp_first = first.data(); a.grp_perm = perm.data(); a.reward = reward.data(); a.scaled = scaled.data(); a.price = price.data();
    a.iters = iters.data(); a.change = change.data(); a.mass = mass.data(); a.samp_reward = rew.data();
    a.samp_action = act.data(); a.samp_price = sprice.data(); a.agree = agree.data(); a.pi = pi.data();
    const int lds = thrl::sp_layout(a);
    printf("G=%d N=%d T=%d D=%d max_iters=%d start_tuple=%d blocks=%d: %d bytes of LDS\n", a.G, a.N, a.T, a.D, a.max_iters,
           a.start_tuple, nblk, lds);
    for (int b = 0; b < nblk; b++) {
        // exactly lds bytes, on the heap: an access past the working set is an access past the allocation
        unsigned char* mem = static_cast<unsigned char*>(aligned_alloc(16, (size_t)lds));
        std::barrier<> bar(thrl::kSpBlock);
        g_bar = &bar;
        std::vector<std::thread> th;
        for (int t = 0; t < thrl::kSpBlock; t++)
            th.emplace_back([&, t] {
                if (a.N <= 2) thrl::sp_block<2>(a, mem, t, b, nblk);
                else thrl::sp_block<thrl::kSpMaxA>(a, mem, t, b, nblk);
            });
        for (auto& x : th) x.join();
        free(mem);
    }
    int bad = cmp("iters", iters, w_iters) + cmp("change", change, w_change) + cmp("mass", mass, w_mass)
        + cmp("samp_reward", rew, w_rew) + cmp("samp_action", act, w_act) + cmp("samp_price", sprice, w_price)
        + cmp("agree", agree, w_agree) + cmp("pi", pi, w_pi);
    printf(bad ? "DIFFERENT from the mirror\n" : "equal to the mirror bit for bit\n");
    return bad ? 1 : 0;
}
