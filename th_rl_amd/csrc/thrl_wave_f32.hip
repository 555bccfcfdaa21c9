// thrl_wave_f32.hip -- instantiates k_wave_episodes<float, *, *, NOISE=false, SWEEP=false, CYCLE=false> (thrl_wave_kernel.h)
#include "thrl_wave_kernel.h"

namespace thrl {

int launch_wave_f32_plain(const WaveArgs& a, int grid, int block, size_t lds, hipStream_t s) {
    // affine payoff grid: closed-form play tables (thrl_wave_f32a.hip); the timing-only ablation builds keep the LUT path they ablate
    if (a.aff_on && !kAblate) return launch_wave_f32_plain_affine(a, grid, block, lds, s);
    return launch_wave_n<float, false, false, false>(a, grid, block, lds, s);
}

}  // namespace thrl
