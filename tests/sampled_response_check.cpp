// sampled_response_check.cpp -- k_sr_response's source (th_rl_amd/csrc/thrl_sampled_response.hip) compiled for the host
// and run as 256 threads with barriers, for address / undefined-behaviour (or thread) sanitizers.  Reads the inputs and
// the mirror's outputs that tests/sampled_response_mirror.write_case writes, runs every game through sr_block and
// compares every output bit for bit.  Built as host code (hipcc -x hip --cuda-host-only -DTHRL_SP_HOST_BUILD), so that
// thrl_solve_dev.h's __host__ __device__ pieces are the ones the device build uses; it makes no HIP call and needs no GPU.
#include "response_check.h"
#include "../th_rl_amd/csrc/thrl_sampled_response.hip"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    auto h = rd<int32_t>(f, 10);             // G N T D agents max_sweeps has_eps_g has_gamma_g has_pi n_blocks
    thrl::SrArgs a;
    memset(&a, 0, sizeof(a));
    thrl::SpArgs& sp = a.sp;
    sp.G = h[0]; sp.N = h[1]; sp.T = h[2]; sp.D = h[3]; a.agents = h[4]; a.max_sweeps = h[5];
    const int nblk = h[9];
    auto kind = rd<int32_t>(f, 8), nact = rd<int32_t>(f, 8);
    auto eps = rd<double>(f, 8), gam = rd<double>(f, 8), tol = rd<double>(f, 1);
    int ts = 1;
    for (int i = sp.N - 1; i >= 0; i--) {
        sp.kind[i] = kind[i]; sp.n_actions[i] = nact[i]; sp.tstride[i] = ts; ts *= nact[i]; sp.eps[i] = eps[i]; a.gamma[i] = gam[i];
    }
    a.eval_tol = tol[0];
    const size_t G = sp.G, N = sp.N, T = sp.T, D = sp.D;
    auto eps_g = rd<double>(f, h[6] ? N * G : 0);
    auto gam_g = rd<double>(f, h[7] ? N * G : 0);
    std::vector<std::vector<float>> prob(N);
    for (size_t i = 0; i < N; i++) prob[i] = rd<float>(f, kind[i] ? G * D * nact[i] : 0);
    auto dpol = rd<uint16_t>(f, G * N * D);
    auto first = rd<int32_t>(f, D + 1), perm = rd<int32_t>(f, T);
    auto reward = rd<double>(f, N * T);
    auto pi = rd<double>(f, h[8] ? G * T : 0);
    auto w_iters = rd<int32_t>(f, N * G), w_sweeps = rd<int32_t>(f, N * G), w_ndiff = rd<int32_t>(f, N * G);
    auto w_lall = rd<double>(f, N * G), w_lmean = rd<double>(f, N * G), w_lw = rd<double>(f, N * G), w_gw = rd<double>(f, N * G),
         w_vw = rd<double>(f, N * G), w_bw = rd<double>(f, N * G);
    auto w_br = rd<uint16_t>(f, N * G * D);
    auto w_vopt = rd<double>(f, N * G * D), w_vpi = rd<double>(f, N * G * D);
    fclose(f);
    // zeroed as the caller's are: the entries of agents that are not selected are not written
    std::vector<int32_t> iters(N * G, 0), sweeps(N * G, 0), ndiff(N * G, 0);
    std::vector<double> lall(N * G, 0.0), lmean(N * G, 0.0), lw(N * G, 0.0), gw(N * G, 0.0), vw(N * G, 0.0), bw(N * G, 0.0);
    std::vector<uint16_t> br(N * G * D, 0);
    std::vector<double> vopt(N * G * D, 0.0), vpi(N * G * D, 0.0);
    sp.eps_g = h[6] ? eps_g.data() : nullptr; a.sweep_gamma = h[7] ? gam_g.data() : nullptr; sp.dpolicy = dpol.data();
    for (size_t i = 0; i < N; i++) sp.prob[i] = kind[i] ? prob[i].data() : nullptr;
    sp.grp_first = first.data(); sp.grp_perm = perm.data(); sp.reward = reward.data();
    a.pi = h[8] ? pi.data() : nullptr;
    a.iters = iters.data(); a.sweeps = sweeps.data(); a.n_diff = ndiff.data();
    a.loss_all = lall.data(); a.loss_mean = lmean.data(); a.loss_w = lw.data(); a.gain_w = gw.data(); a.v_w = vw.data();
    a.br_prob_w = bw.data(); a.br_policy = br.data(); a.v_opt = vopt.data(); a.v_pi = vpi.data();
    const long long lds = thrl::sr_layout(a);
    printf("G=%d N=%d T=%d D=%d agents=0x%x max_sweeps=%d blocks=%d team=%d: %lld bytes of LDS\n", sp.G, sp.N, sp.T, sp.D, a.agents,
           a.max_sweeps, nblk, a.team, lds);
    run_blocks(lds, nblk, thrl::kSpBlock, [&](unsigned char* mem, int t, int b) {
        if (sp.N <= 2) thrl::sr_block<2>(a, mem, t, b, nblk);
        else thrl::sr_block<thrl::kSpMaxA>(a, mem, t, b, nblk);
    });
    int bad = cmp("iters", iters, w_iters) + cmp("sweeps", sweeps, w_sweeps) + cmp("n_diff", ndiff, w_ndiff)
        + cmp("loss_all", lall, w_lall) + cmp("loss_mean", lmean, w_lmean) + cmp("loss_w", lw, w_lw) + cmp("gain_w", gw, w_gw)
        + cmp("v_w", vw, w_vw) + cmp("br_prob_w", bw, w_bw) + cmp("br_policy", br, w_br) + cmp("v_opt", vopt, w_vopt)
        + cmp("v_pi", vpi, w_vpi);
    printf(bad ? "DIFFERENT from the mirror\n" : "equal to the mirror bit for bit\n");
    return bad ? 1 : 0;
}
