// sampled_deviation_noise_check.cpp -- k_sdn_chain's source (th_rl_amd/csrc/thrl_sampled_deviation_noise.hip) compiled
// for the host and run as 256 threads with barriers, for address / undefined-behaviour (or thread) sanitizers.  Reads the
// inputs and the mirror's outputs that tests/sampled_deviation_noise_mirror.write_case writes, runs every game through
// sdn_block and compares every output bit for bit.  Built as host code (hipcc -x hip --cuda-host-only
// -DTHRL_SP_HOST_BUILD), so that thrl_solve_dev.h's __host__ __device__ pieces are the ones the device build uses; it
// makes no HIP call and needs no GPU.  What it shares with sampled_deviation_check.cpp is in deviation_check.h.
#include "deviation_check.h"
#include "../th_rl_amd/csrc/thrl_sampled_deviation_noise.hip"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    SdCase c{fopen(argv[1], "rb")};
    if (!c.f) return 2;
    // G N T D Jn W deviator dev_len n_steps dev_action has_dev_policy has_eps_g has_gamma_g has_noise_g row_begin row_count
    // n_blocks
    auto h = rd<int32_t>(c.f, 17);
    thrl::SdnArgs a;
    memset(&a, 0, sizeof(a));
    thrl::SpnArgs& na = a.n;
    thrl::SpArgs& sp = na.sp;
    thrl::SdArgs& sd = a.sd;
    sp.G = h[0]; sp.N = h[1]; sp.T = h[2]; sp.D = h[3]; na.Jn = h[4]; na.W = h[5];
    sd.d = h[6]; sd.L = h[7]; sd.K = h[8]; sd.dev_action = h[9]; sd.use_policy = h[10]; sd.row_begin = h[14]; sd.row_count = h[15];
    const int nblk = h[16];
    c.agents(sp, sd, 3, h[11], h[12]);
    na.noise_prob = c.scalars[2];
    const size_t G = c.G, N = c.N, T = c.T, D = c.D, Jn = na.Jn, W = na.W;
    auto p_g = rd<double>(c.f, h[13] ? G : 0);
    c.rows();
    // the node rows one float off a 16-byte boundary, as a game's rows fall in the device's array
    std::vector<std::vector<float>> nprob(N);
    for (size_t i = 0; i < N; i++) {
        auto v = rd<float>(c.f, c.kind[i] ? G * Jn * c.nact[i] : 0);
        nprob[i].assign(v.size() + 1, 0.0f);
        std::copy(v.begin(), v.end(), nprob[i].begin() + 1);
    }
    c.dpol = rd<uint16_t>(c.f, G * N * D);
    auto npol = rd<uint16_t>(c.f, G * N * Jn);
    c.devpol = rd<uint16_t>(c.f, h[10] ? G * (D + Jn) : 0);
    c.tables();
    auto band_lo = rd<int32_t>(c.f, T);
    auto band = rd<double>(c.f, T * W), nprice = rd<double>(c.f, T), nreward = rd<double>(c.f, N * T);
    c.expected();
    c.bind(sp, sd);
    na.noise_prob_g = h[13] ? p_g.data() : nullptr;
    na.npolicy = npol.data();
    for (size_t i = 0; i < N; i++) na.nprob[i] = c.kind[i] ? nprob[i].data() + 1 : nullptr;
    na.band_lo = band_lo.data(); na.band = band.data(); na.noise_price = nprice.data(); na.noise_reward = nreward.data();
    const long long lds = thrl::sdn_layout(a);
    printf("G=%d N=%d T=%d D=%d Jn=%d W=%d deviator=%d L=%d K=%d dev_action=%d policy=%d rows [%d, +%d) blocks=%d: %lld bytes of LDS\n",
           sp.G, sp.N, sp.T, sp.D, na.Jn, na.W, sd.d, sd.L, sd.K, sd.dev_action, sd.use_policy, sd.row_begin, sd.row_count, nblk, lds);
    run_blocks(lds, nblk, thrl::kSpBlock, [&](unsigned char* mem, int t, int b) {
        if (sp.N <= 2) thrl::sdn_block<2>(a, mem, t, b, nblk);
        else thrl::sdn_block<thrl::kSpMaxA>(a, mem, t, b, nblk);
    });
    return c.compare();
}
