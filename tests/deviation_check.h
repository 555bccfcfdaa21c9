// deviation_check.h -- what tests/sampled_deviation_check.cpp and tests/sampled_deviation_noise_check.cpp share on top of
// response_check.h: the shims under which a deviation kernel's source compiles for the host (include this, then the
// kernel's .hip), and SdCase: the inputs, the mirror's outputs and the poisoned outputs that both case files hold, read in
// the files' order by the stages below (a program reads what only its own file has between them), the binding of SpArgs'
// and SdArgs' pointers and the comparison.
#pragma once
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
#include "../th_rl_amd/csrc/thrl_sampled_deviation.h"

struct SdCase {
    FILE* f;
    size_t G = 0, N = 0, T = 0, D = 0, R = 0;
    std::vector<int32_t> kind, nact, first, perm, w_lstep, w_ret, lstep, ret;
    std::vector<double> scalars, eps_g, gam_g, reward, scaled, price, weights;
    std::vector<std::vector<float>> prob;
    std::vector<uint16_t> dpol, devpol;
    // the mirror's outputs, and the program's in the same order
    std::vector<double> w_brew, w_bact, w_bprice, w_share, w_gain, w_gdev, w_low, w_dist, w_mass, w_rrows, w_arows, w_prows, w_drows;
    std::vector<double> brew, bact, bprice, share, gain, gdev, low, dist, mass, rrows, arows, prows, drows;

    // the agents' kinds, action counts and epsilons into sp (whose counts and sd's row_count the caller has set), the
    // n_scalars scalars (gamma, ret_tol and what the call adds), then the per-game epsilons and gammas
    void agents(thrl::SpArgs& sp, thrl::SdArgs& sd, size_t n_scalars, bool has_eps_g, bool has_gam_g) {
        G = sp.G; N = sp.N; T = sp.T; D = sp.D; R = sd.row_count;
        kind = rd<int32_t>(f, 8); nact = rd<int32_t>(f, 8);
        auto eps = rd<double>(f, 8);
        scalars = rd<double>(f, n_scalars);
        int ts = 1;
        for (int i = sp.N - 1; i >= 0; i--) {
            sp.kind[i] = kind[i]; sp.n_actions[i] = nact[i]; sp.tstride[i] = ts; ts *= nact[i]; sp.eps[i] = eps[i];
        }
        sd.gamma = scalars[0]; sd.ret_tol = scalars[1];
        eps_g = rd<double>(f, has_eps_g ? N * G : 0);
        gam_g = rd<double>(f, has_gam_g ? N * G : 0);
    }
    // the networks' rows at the distinct prices
    void rows() {
        prob.resize(N);
        for (size_t i = 0; i < N; i++) prob[i] = rd<float>(f, kind[i] ? G * D * nact[i] : 0);
    }
    void tables() {
        first = rd<int32_t>(f, D + 1); perm = rd<int32_t>(f, T);
        reward = rd<double>(f, N * T); scaled = rd<double>(f, N * T); price = rd<double>(f, T);
    }
    // x_0, the mirror's outputs (the end of the file) and the program's own
    void expected() {
        weights = rd<double>(f, G * T);
        w_brew = rd<double>(f, N * G); w_bact = rd<double>(f, N * G);
        for (auto* v : {&w_bprice, &w_share, &w_gain, &w_gdev, &w_low, &w_dist, &w_mass}) *v = rd<double>(f, G);
        w_lstep = rd<int32_t>(f, G); w_ret = rd<int32_t>(f, G);
        w_rrows = rd<double>(f, R * N * G); w_arows = rd<double>(f, R * N * G);
        w_prows = rd<double>(f, R * G); w_drows = rd<double>(f, R * G);
        fclose(f);
        // poisoned, not zeroed: the call writes every entry of every output
        const double poison = -7.25;
        brew.assign(N * G, poison); bact.assign(N * G, poison);
        for (auto* v : {&bprice, &share, &gain, &gdev, &low, &dist, &mass}) v->assign(G, poison);
        rrows.assign(R * N * G, poison); arows.assign(R * N * G, poison); prows.assign(R * G, poison); drows.assign(R * G, poison);
        lstep.assign(G, -7); ret.assign(G, -7);
    }
    void bind(thrl::SpArgs& sp, thrl::SdArgs& sd) {
        sp.eps_g = eps_g.empty() ? nullptr : eps_g.data(); sd.sweep_gamma = gam_g.empty() ? nullptr : gam_g.data();
        sp.dpolicy = dpol.data(); sd.dev_policy = sd.use_policy ? devpol.data() : nullptr;
        for (size_t i = 0; i < N; i++) sp.prob[i] = kind[i] ? prob[i].data() : nullptr;
        sp.grp_first = first.data(); sp.grp_perm = perm.data(); sp.reward = reward.data(); sp.scaled = scaled.data();
        sp.price = price.data();
        sd.weights = weights.data();
        sd.base_reward = brew.data(); sd.base_action = bact.data(); sd.base_price = bprice.data(); sd.dev_share = share.data();
        sd.gain = gain.data(); sd.gain_dev = gdev.data(); sd.low = low.data(); sd.dist = dist.data(); sd.mass = mass.data();
        sd.low_step = lstep.data(); sd.ret_step = ret.data();
        sd.reward_rows = rrows.data(); sd.action_rows = arows.data(); sd.price_rows = prows.data(); sd.dist_rows = drows.data();
    }
    // the program's exit status
    int compare() const {
        int bad = cmp("base_reward", brew, w_brew) + cmp("base_action", bact, w_bact) + cmp("base_price", bprice, w_bprice)
            + cmp("dev_share", share, w_share) + cmp("gain", gain, w_gain) + cmp("gain_dev", gdev, w_gdev) + cmp("low", low, w_low)
            + cmp("dist", dist, w_dist) + cmp("mass", mass, w_mass) + cmp("low_step", lstep, w_lstep) + cmp("ret_step", ret, w_ret)
            + cmp("reward_rows", rrows, w_rrows) + cmp("action_rows", arows, w_arows) + cmp("price_rows", prows, w_prows)
            + cmp("dist_rows", drows, w_drows);
        printf(bad ? "DIFFERENT from the mirror\n" : "equal to the mirror bit for bit\n");
        return bad ? 1 : 0;
    }
};
