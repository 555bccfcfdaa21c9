// sampled_deviation_noise_check.cpp -- k_sdn_chain's source (th_rl_amd/csrc/thrl_sampled_deviation_noise.hip) compiled
// for the host and run as 256 threads with barriers, for address / undefined-behaviour (or thread) sanitizers.  Reads the
// inputs and the mirror's outputs that tests/sampled_deviation_noise_mirror.write_case writes, runs every game through
// sdn_block and compares every output bit for bit.  Built as host code (hipcc -x hip --cuda-host-only
// -DTHRL_SP_HOST_BUILD), so that thrl_solve_dev.h's __host__ __device__ pieces are the ones the device build uses; it
// makes no HIP call and needs no GPU.
#include <cmath>
#include <hip/hip_runtime.h>
// thrl_chain_dev.h's read-back as host code: response_check.h's first include would bring it as HIP declares it, as device
// functions, before its shims stand
#pragma push_macro("__device__")
#undef __device__
#define __device__
#define __dadd_rn(a, b) ((a) + (b))
#define __dsub_rn(a, b) ((a) - (b))
#define __dmul_rn(a, b) ((a) * (b))
#include "../th_rl_amd/csrc/thrl_chain_dev.h"
#undef __dadd_rn
#undef __dsub_rn
#undef __dmul_rn
#pragma pop_macro("__device__")
#include "response_check.h"
#include "../th_rl_amd/csrc/thrl_sampled_deviation_noise.hip"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    // G N T D Jn W deviator dev_len n_steps dev_action has_dev_policy has_eps_g has_gamma_g has_noise_g row_begin row_count
    // n_blocks
    auto h = rd<int32_t>(f, 17);
    thrl::SdnArgs a;
    memset(&a, 0, sizeof(a));
    thrl::SpnArgs& na = a.n;
    thrl::SpArgs& sp = na.sp;
    thrl::SdArgs& sd = a.sd;
    sp.G = h[0]; sp.N = h[1]; sp.T = h[2]; sp.D = h[3]; na.Jn = h[4]; na.W = h[5];
    sd.d = h[6]; sd.L = h[7]; sd.K = h[8]; sd.dev_action = h[9]; sd.use_policy = h[10]; sd.row_begin = h[14]; sd.row_count = h[15];
    const int nblk = h[16];
    auto kind = rd<int32_t>(f, 8), nact = rd<int32_t>(f, 8);
    auto eps = rd<double>(f, 8), gr = rd<double>(f, 3);
    int ts = 1;
    for (int i = sp.N - 1; i >= 0; i--) {
        sp.kind[i] = kind[i]; sp.n_actions[i] = nact[i]; sp.tstride[i] = ts; ts *= nact[i]; sp.eps[i] = eps[i];
    }
    sd.gamma = gr[0]; sd.ret_tol = gr[1]; na.noise_prob = gr[2];
    const size_t G = sp.G, N = sp.N, T = sp.T, D = sp.D, Jn = na.Jn, W = na.W, R = sd.row_count;
    auto eps_g = rd<double>(f, h[11] ? N * G : 0);
    auto gam_g = rd<double>(f, h[12] ? N * G : 0);
    auto p_g = rd<double>(f, h[13] ? G : 0);
    std::vector<std::vector<float>> prob(N), nprob(N);
    for (size_t i = 0; i < N; i++) prob[i] = rd<float>(f, kind[i] ? G * D * nact[i] : 0);
    // the node rows one float off a 16-byte boundary, as a game's rows fall in the device's array
    for (size_t i = 0; i < N; i++) {
        auto v = rd<float>(f, kind[i] ? G * Jn * nact[i] : 0);
        nprob[i].assign(v.size() + 1, 0.0f);
        std::copy(v.begin(), v.end(), nprob[i].begin() + 1);
    }
    auto dpol = rd<uint16_t>(f, G * N * D), npol = rd<uint16_t>(f, G * N * Jn);
    auto devpol = rd<uint16_t>(f, h[10] ? G * (D + Jn) : 0);
    auto first = rd<int32_t>(f, D + 1), perm = rd<int32_t>(f, T);
    auto reward = rd<double>(f, N * T), scaled = rd<double>(f, N * T), price = rd<double>(f, T);
    auto band_lo = rd<int32_t>(f, T);
    auto band = rd<double>(f, T * W), nprice = rd<double>(f, T), nreward = rd<double>(f, N * T);
    auto weights = rd<double>(f, G * T);
    auto w_brew = rd<double>(f, N * G), w_bact = rd<double>(f, N * G);
    auto w_bprice = rd<double>(f, G), w_share = rd<double>(f, G), w_gain = rd<double>(f, G), w_gdev = rd<double>(f, G),
         w_low = rd<double>(f, G), w_dist = rd<double>(f, G), w_mass = rd<double>(f, G);
    auto w_lstep = rd<int32_t>(f, G), w_ret = rd<int32_t>(f, G);
    auto w_rrows = rd<double>(f, R * N * G), w_arows = rd<double>(f, R * N * G), w_prows = rd<double>(f, R * G),
         w_drows = rd<double>(f, R * G);
    fclose(f);
    // poisoned, not zeroed: the call writes every entry of every output
    const double poison = -7.25;
    std::vector<double> brew(N * G, poison), bact(N * G, poison), bprice(G, poison), share(G, poison), gain(G, poison),
        gdev(G, poison), low(G, poison), dist(G, poison), mass(G, poison), rrows(R * N * G, poison), arows(R * N * G, poison),
        prows(R * G, poison), drows(R * G, poison);
    std::vector<int32_t> lstep(G, -7), ret(G, -7);
    sp.eps_g = h[11] ? eps_g.data() : nullptr; sd.sweep_gamma = h[12] ? gam_g.data() : nullptr;
    na.noise_prob_g = h[13] ? p_g.data() : nullptr;
    sp.dpolicy = dpol.data(); na.npolicy = npol.data();
    sd.dev_policy = h[10] ? devpol.data() : nullptr;
    for (size_t i = 0; i < N; i++) {
        sp.prob[i] = kind[i] ? prob[i].data() : nullptr;
        na.nprob[i] = kind[i] ? nprob[i].data() + 1 : nullptr;
    }
    sp.grp_first = first.data(); sp.grp_perm = perm.data(); sp.reward = reward.data(); sp.scaled = scaled.data();
    sp.price = price.data();
    na.band_lo = band_lo.data(); na.band = band.data(); na.noise_price = nprice.data(); na.noise_reward = nreward.data();
    sd.weights = weights.data();
    sd.base_reward = brew.data(); sd.base_action = bact.data(); sd.base_price = bprice.data(); sd.dev_share = share.data();
    sd.gain = gain.data(); sd.gain_dev = gdev.data(); sd.low = low.data(); sd.dist = dist.data(); sd.mass = mass.data();
    sd.low_step = lstep.data(); sd.ret_step = ret.data();
    sd.reward_rows = rrows.data(); sd.action_rows = arows.data(); sd.price_rows = prows.data(); sd.dist_rows = drows.data();
    const long long lds = thrl::sdn_layout(a);
    printf("G=%d N=%d T=%d D=%d Jn=%d W=%d deviator=%d L=%d K=%d dev_action=%d policy=%d rows [%d, +%d) blocks=%d: %lld bytes of LDS\n",
           sp.G, sp.N, sp.T, sp.D, na.Jn, na.W, sd.d, sd.L, sd.K, sd.dev_action, sd.use_policy, sd.row_begin, sd.row_count, nblk, lds);
    run_blocks(lds, nblk, thrl::kSpBlock, [&](unsigned char* mem, int t, int b) {
        if (sp.N <= 2) thrl::sdn_block<2>(a, mem, t, b, nblk);
        else thrl::sdn_block<thrl::kSpMaxA>(a, mem, t, b, nblk);
    });
    int bad = cmp("base_reward", brew, w_brew) + cmp("base_action", bact, w_bact) + cmp("base_price", bprice, w_bprice)
        + cmp("dev_share", share, w_share) + cmp("gain", gain, w_gain) + cmp("gain_dev", gdev, w_gdev) + cmp("low", low, w_low)
        + cmp("dist", dist, w_dist) + cmp("mass", mass, w_mass) + cmp("low_step", lstep, w_lstep) + cmp("ret_step", ret, w_ret)
        + cmp("reward_rows", rrows, w_rrows) + cmp("action_rows", arows, w_arows) + cmp("price_rows", prows, w_prows)
        + cmp("dist_rows", drows, w_drows);
    printf(bad ? "DIFFERENT from the mirror\n" : "equal to the mirror bit for bit\n");
    return bad ? 1 : 0;
}
