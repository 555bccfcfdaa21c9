// sampled_deviation_check.cpp -- k_sd_chain's source (th_rl_amd/csrc/thrl_sampled_deviation.hip) compiled for the host
// and run as 256 threads with barriers, for address / undefined-behaviour (or thread) sanitizers.  Reads the inputs and
// the mirror's outputs that tests/sampled_deviation_mirror.write_case writes, runs every game through sd_block and
// compares every output bit for bit.  Built as host code (hipcc -x hip --cuda-host-only -DTHRL_SP_HOST_BUILD), so that
// thrl_solve_dev.h's __host__ __device__ pieces are the ones the device build uses; it makes no HIP call and needs no GPU.
// What it shares with sampled_deviation_noise_check.cpp is in deviation_check.h.
#include "deviation_check.h"
#include "../th_rl_amd/csrc/thrl_sampled_deviation.hip"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    SdCase c{fopen(argv[1], "rb")};
    if (!c.f) return 2;
    // G N T D deviator dev_len n_steps dev_action has_dev_policy has_eps_g has_gamma_g row_begin row_count n_blocks
    auto h = rd<int32_t>(c.f, 14);
    thrl::SdArgs a;
    memset(&a, 0, sizeof(a));
    thrl::SpArgs& sp = a.sp;
    sp.G = h[0]; sp.N = h[1]; sp.T = h[2]; sp.D = h[3];
    a.d = h[4]; a.L = h[5]; a.K = h[6]; a.dev_action = h[7]; a.use_policy = h[8]; a.row_begin = h[11]; a.row_count = h[12];
    const int nblk = h[13];
    c.agents(sp, a, 2, h[9], h[10]);
    c.rows();
    c.dpol = rd<uint16_t>(c.f, c.G * c.N * c.D);
    c.devpol = rd<uint16_t>(c.f, h[8] ? c.G * c.D : 0);
    c.tables();
    c.expected();
    c.bind(sp, a);
    const long long lds = thrl::sd_layout(a);
    printf("G=%d N=%d T=%d D=%d deviator=%d L=%d K=%d dev_action=%d policy=%d rows [%d, +%d) blocks=%d: %lld bytes of LDS\n", sp.G, sp.N,
           sp.T, sp.D, a.d, a.L, a.K, a.dev_action, a.use_policy, a.row_begin, a.row_count, nblk, lds);
    run_blocks(lds, nblk, thrl::kSpBlock, [&](unsigned char* mem, int t, int b) {
        if (sp.N <= 2) thrl::sd_block<2>(a, mem, t, b, nblk);
        else thrl::sd_block<thrl::kSpMaxA>(a, mem, t, b, nblk);
    });
    return c.compare();
}
