// thrl_wave_f32a.hip -- instantiates k_wave_episodes<float, 1..4, 1, NOISE=false, SWEEP=false, CYCLE=false, GREEDY=false, LOG, AFFINE=true>
// (thrl_wave_kernel.h): the plain float32 variants with closed-form play tables, for payoff grids on which the next row is affine
// in the two action indices (WaveArgs.aff_on, decided by plan_wave in thrl_api.hip)
#include "thrl_wave_kernel.h"

namespace thrl {

template <bool LOG>
static int launch_affine(const WaveArgs& a, int grid, int block, size_t lds, hipStream_t s) {
    switch ((a.T + 63) / 64) {
        case 1: return launch_wave_t<float, 1, 1, false, false, false, false, LOG, true>(a, grid, block, lds, s);
        case 2: return launch_wave_t<float, 2, 1, false, false, false, false, LOG, true>(a, grid, block, lds, s);
        case 3: return launch_wave_t<float, 3, 1, false, false, false, false, LOG, true>(a, grid, block, lds, s);
        case 4: return launch_wave_t<float, 4, 1, false, false, false, false, LOG, true>(a, grid, block, lds, s);
    }
    return -1;
}

int launch_wave_f32_plain_affine(const WaveArgs& a, int grid, int block, size_t lds, hipStream_t s) {
    if (!a.aff_on || a.win_rows + 2 > 64 || a.epk != 1 || a.replay_from != 0) return -1;      // (the plan never asks for it then)
    if (a.game_reward_log || a.game_action_log) return launch_affine<true>(a, grid, block, lds, s);
    return launch_affine<false>(a, grid, block, lds, s);
}

}  // namespace thrl
