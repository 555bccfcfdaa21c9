// sampled_noise_host_check.cpp -- k_spn_chain's and k_spn_jump's source (th_rl_amd/csrc/thrl_sampled_noise.hip) compiled
// for the host and run as 256 threads with barriers, for address / undefined-behaviour sanitizers.  Reads the inputs and
// the mirror's outputs that profiles/sampled_noise_host_check.py writes, runs every game through spn_block and compares
// every output bit for bit.  LDS is a heap block of exactly the planned size, and every input array is a heap block of
// exactly its size, so a read outside the working set or outside a row is a read outside an allocation.
// Build and run: see profiles/sampled_noise_host_check.py.  No GPU is involved.
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

#include "thrl_sampled_noise.hip"

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
    auto h = rd<int32_t>(f, 12);             // G N T D Jn W max_iters start(0 uniform, 1 tuples, 2 reset) has_eps_g has_p_g n_blocks shift
    thrl::SpnArgs a;
    memset(&a, 0, sizeof(a));
    thrl::SpArgs& sa = a.sp;
    sa.G = h[0]; sa.N = h[1]; sa.T = h[2]; sa.D = h[3]; a.Jn = h[4]; a.W = h[5]; sa.max_iters = h[6];
    sa.start_tuple = h[7] == 1; a.start_reset = h[7] == 2;
    const int nblk = h[10], shift = h[11];   // shift: floats the node rows are moved off their allocation's alignment
    auto kind = rd<int32_t>(f, 8), nact = rd<int32_t>(f, 8);
    auto eps = rd<double>(f, 8), tolp = rd<double>(f, 2);
    int ts = 1;
    for (int i = sa.N - 1; i >= 0; i--) {
        sa.kind[i] = kind[i]; sa.n_actions[i] = nact[i]; sa.tstride[i] = ts; ts *= nact[i]; sa.eps[i] = eps[i];
    }
    sa.tol = tolp[0]; a.noise_prob = tolp[1];
    const size_t G = sa.G, N = sa.N, T = sa.T, D = sa.D, Jn = a.Jn, W = a.W;
    auto eps_g = rd<double>(f, h[8] ? N * G : 0);
    auto p_g = rd<double>(f, h[9] ? G : 0);
    auto start = rd<int32_t>(f, G);
    std::vector<std::vector<float>> prob(N), nprob(N);
    for (size_t i = 0; i < N; i++) prob[i] = rd<float>(f, kind[i] ? G * D * nact[i] : 0);
    for (size_t i = 0; i < N; i++) {
        auto v = rd<float>(f, kind[i] ? G * Jn * nact[i] : 0);
        nprob[i].assign(v.size() + (kind[i] ? shift : 0), 0.0f);     // the rows end where the allocation ends
        std::copy(v.begin(), v.end(), nprob[i].begin() + (kind[i] ? shift : 0));
    }
    auto dpol = rd<uint16_t>(f, G * N * D), npol = rd<uint16_t>(f, G * N * Jn);
    auto first = rd<int32_t>(f, D + 1), perm = rd<int32_t>(f, T);
    auto reward = rd<double>(f, N * T), scaled = rd<double>(f, N * T), price = rd<double>(f, T);
    auto band_lo = rd<int32_t>(f, T);
    auto band = rd<double>(f, T * W), nprice = rd<double>(f, T), nreward = rd<double>(f, N * T), node_w = rd<double>(f, Jn);
    auto w_iters = rd<int32_t>(f, G);
    auto w_change = rd<double>(f, G), w_mass = rd<double>(f, G), w_rew = rd<double>(f, N * G), w_act = rd<double>(f, N * G),
         w_price = rd<double>(f, G), w_agree = rd<double>(f, G), w_pi = rd<double>(f, G * T), w_jump = rd<double>(f, G);
    fclose(f);
    std::vector<int32_t> iters(G, -7);
    std::vector<double> change(G, -7), mass(G, -7), rew(N * G, -7), act(N * G, -7), sprice(G, -7), agree(G, -7), pi(G * T, -7),
        jump(G, -7);
    sa.eps_g = h[8] ? eps_g.data() : nullptr; sa.start = start.data(); sa.dpolicy = dpol.data();
    a.noise_prob_g = h[9] ? p_g.data() : nullptr; a.npolicy = npol.data();
    for (size_t i = 0; i < N; i++) {
        sa.prob[i] = kind[i] ? prob[i].data() : nullptr;
        a.nprob[i] = kind[i] ? nprob[i].data() + shift : nullptr;
    }
    sa.grp_first = first.data(); sa.grp_perm = perm.data(); sa.reward = reward.data(); sa.scaled = scaled.data(); sa.price = price.data();
    a.band_lo = band_lo.data(); a.band = band.data(); a.noise_price = nprice.data(); a.noise_reward = nreward.data();
    a.node_w = node_w.data(); a.max_jump = jump.data();
    sa.iters = iters.data(); sa.change = change.data(); sa.mass = mass.data(); sa.samp_reward = rew.data();
    sa.samp_action = act.data(); sa.samp_price = sprice.data(); sa.agree = agree.data(); sa.pi = pi.data();
    const int lds = (int)thrl::spn_layout(a);
    printf("G=%d N=%d T=%d D=%d Jn=%d W=%d max_iters=%d start=%d blocks=%d shift=%d: %d bytes of LDS\n", sa.G, sa.N, sa.T, sa.D,
           a.Jn, a.W, sa.max_iters, h[7], nblk, shift, lds);
    for (int b = 0; b < nblk; b++) {
        // exactly lds bytes, on the heap: an access past the working set is an access past the allocation
        unsigned char* mem = static_cast<unsigned char*>(aligned_alloc(16, (size_t)lds));
        std::vector<double> red(thrl::kSpBlock);
        std::barrier<> bar(thrl::kSpBlock);
        g_bar = &bar;
        std::vector<std::thread> th;
        for (int t = 0; t < thrl::kSpBlock; t++)
            th.emplace_back([&, t] {
                thrl::spn_jump_block(a, red.data(), t, b, nblk);
                if (sa.N <= 2) thrl::spn_block<2>(a, mem, t, b, nblk);
                else thrl::spn_block<thrl::kSpMaxA>(a, mem, t, b, nblk);
            });
        for (auto& x : th) x.join();
        free(mem);
    }
    int bad = cmp("iters", iters, w_iters) + cmp("change", change, w_change) + cmp("mass", mass, w_mass)
        + cmp("samp_reward", rew, w_rew) + cmp("samp_action", act, w_act) + cmp("samp_price", sprice, w_price)
        + cmp("agree", agree, w_agree) + cmp("pi", pi, w_pi) + cmp("max_jump", jump, w_jump);
    printf(bad ? "DIFFERENT from the mirror\n" : "equal to the mirror bit for bit\n");
    return bad ? 1 : 0;
}
