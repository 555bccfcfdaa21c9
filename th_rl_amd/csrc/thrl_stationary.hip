// thrl_stationary.hip -- greedy play under demand noise (thrl_stationary, include/thrl.h): the long-run distribution
// of a game's noisy greedy play over the price cells, by lazy power iteration of its Markov chain, and the reward,
// action and price that distribution earns.
//
// One wavefront (a one-wave block) per game, looping over games, lanes owning TARGET cells k = lane, lane + 64, ...
// Per game the wave gathers the policy entries of the cells' rows (2 bytes each) into the tuple of every cell and
// stages, per cell, the deterministic successor and the place of the tuple's band row; both iterates live in LDS.  A
// step is target-major: every lane walks the sources j in ascending order, reads mu(j) and the source's det / band
// place as LDS broadcasts and its own band entry from global memory (consecutive lanes, consecutive addresses; the
// band table is shared by all games and stays in L2), so the order of the adds is the definition's whatever the
// scheduling, and no atomic is involved.  A lane carries two targets (k, k + 64) through one walk.  The ordered
// output sums follow k_attractors: chunks of 64 cells, one lane per cell for the products, then one lane per output
// reading them back from LDS in ascending k.
#include "thrl_stationary.h"
#include "thrl_solve_dev.h"

namespace thrl {

namespace {

struct StatCell {           // what a step needs of source cell j
    int det;                // its deterministic successor cell
    int blo;                // band_lo of its tuple
    uint32_t boff;          // t * W - band_lo: band index of target k = boff + k (mod 2^32) when 0 <= k - blo < W
};

template <bool kCellLds>
__global__ void __launch_bounds__(64) k_stationary(const StatArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    const int lane = threadIdx.x;
    const int N = a.N, G = a.G, J = a.J, W = a.W, TT = a.T;
    double* mua = reinterpret_cast<double*>(s_mem + a.o_mua);
    double* mub = reinterpret_cast<double*>(s_mem + a.o_mub);
    double* prod = reinterpret_cast<double*>(s_mem + a.o_prod);       // [2N + 2][64] the chunk's terms per output
    // the per-cell tables exist only in the <true> variant: without them their offsets coincide with tup's
    uint32_t* boff = kCellLds ? reinterpret_cast<uint32_t*>(s_mem + a.o_boff) : nullptr;
    int32_t* blo = kCellLds ? reinterpret_cast<int32_t*>(s_mem + a.o_blo) : nullptr;
    uint16_t* det = kCellLds ? reinterpret_cast<uint16_t*>(s_mem + a.o_det) : nullptr;
    uint16_t* tup = reinterpret_cast<uint16_t*>(s_mem + a.o_tup);
    const int n_out = 2 * N + 2;                                      // mass, N rewards, N actions, price

    auto cell = [&](int j) -> StatCell {
        if constexpr (kCellLds) return StatCell{(int)det[j], blo[j], boff[j]};
        const int t = tup[j];
        const int b = a.band_lo[t];
        const int d = a.det_cell[t];
        return StatCell{(d >= 0 && d < J) ? d : 0xffff, b, (uint32_t)(t * W) - (uint32_t)b};
    };

    for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
        const uint16_t* __restrict__ pg = a.policy + g * a.P;
        const double p = a.noise_prob_g ? a.noise_prob_g[g] : a.noise_prob;
        const double q = __dsub_rn(1.0, p);
        bool ok = p > 0.0 && p <= 1.0;

        // ---- the tuple of every cell, and the start cell
        int found = -1;
        double st = 0.0;
        if (a.start_state) st = a.state0[g];
        for (int k = lane; k < J; k += 64) {
            int t = 0;
            bool eq = true;
            for (int i = 0; i < N; i++) {
                const int row = clamp_row(a.cell_rows[(int64_t)i * J + k], a.ag[i]);
                t += row_action(a, pg, i, row) * a.tstride[i];
                if (a.start_state) eq = eq && row == encode64(st, a.ag[i]);
            }
            tup[k] = (uint16_t)t;
            if constexpr (kCellLds) {
                const int b = a.band_lo[t];
                const int d = a.det_cell[t];
                det[k] = (uint16_t)((d >= 0 && d < J) ? d : 0xffff);
                blo[k] = b;
                boff[k] = (uint32_t)(t * W) - (uint32_t)b;
            }
            if (a.start_state && eq && found < 0) found = k;
        }
        int k_start = -1;
        if (a.start_state) {
            // the first cell with x_0's rows: the lowest k over the lanes
            int best = found >= 0 ? found : 0x7fffffff;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) best = min(best, __shfl_xor(best, m));
            k_start = best;
            ok = ok && best < J;
        }
        if (!ok) {                                       // wave-uniform: this game is not solved
            chain_unsolved(a.iters, a.change, a.mass, a.stat_price, a.stat_reward, a.stat_action, a.pi, g, G, N, J, lane, 64);
            __syncthreads();
            continue;
        }
        for (int k = lane; k < J; k += 64) mua[k] = a.start_state ? (k == k_start ? 1.0 : 0.0) : a.cell_w[k];
        __syncthreads();

        // ---- mu' = mu / 2 + (mu P) / 2 until the largest change is within tol
        double* mo = mua;
        double* mn = mub;
        int it = 0;
        double chg = 0.0;
        for (;;) {
            double c = 0.0;
            for (int k0 = lane; k0 < J; k0 += 128) {
                const int k1 = k0 + 64;
                double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
                for (int j = 0; j < J; j++) {
                    const double m = mo[j];
                    if (m == 0.0) continue;              // the terms are +0.0: adding them changes nothing
                    const StatCell sc = cell(j);
                    const uint32_t d0 = (uint32_t)(k0 - sc.blo), d1 = (uint32_t)(k1 - sc.blo);
                    const double n0 = d0 < (uint32_t)W ? a.band[sc.boff + (uint32_t)k0] : 0.0;
                    const double n1 = (d1 < (uint32_t)W && k1 < J) ? a.band[sc.boff + (uint32_t)k1] : 0.0;
                    const double pn0 = __dmul_rn(p, n0), pn1 = __dmul_rn(p, n1);
                    const double P0 = sc.det == k0 ? __dadd_rn(q, pn0) : pn0;
                    const double P1 = sc.det == k1 ? __dadd_rn(q, pn1) : pn1;
                    if (P0 != 0.0) s0 = __dadd_rn(s0, __dmul_rn(m, P0));
                    if (P1 != 0.0) s1 = __dadd_rn(s1, __dmul_rn(m, P1));
                }
                mn[k0] = chain_lazy(mo[k0], s0, c);
                if (k1 < J) mn[k1] = chain_lazy(mo[k1], s1, c);
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) c = fmax(c, __shfl_xor(c, m));
            __syncthreads();
            double* tm = mo; mo = mn; mn = tm;
            it++;
            chg = c;
            if (c <= a.tol || it >= a.max_iters) break;
        }

        // ---- the outputs: chunks of 64 cells, one lane per cell, then one lane per ordered sum
        double acc = 0.0;
        for (int k0 = 0; k0 < J; k0 += 64) {
            const int k = k0 + lane;
            if (k < J) {
                const int t = tup[k];
                const double m = mo[k];
                double sc[THRL_MAXA], rw[THRL_MAXA];
                int rest = t;
                for (int i = 0; i < N; i++) {
                    const int ai = rest / a.tstride[i];
                    rest -= ai * a.tstride[i];
                    sc[i] = scale_action(ai, a.ag[i]);
                }
                const double price = env_step<THRL_MAXA>(a.env, N, sc, a.env.a, rw);
                prod[lane] = m;
                for (int i = 0; i < N; i++) {
                    const double r = a.rew[(int64_t)i * TT + t], nr = a.noise_reward[(int64_t)i * TT + t];
                    prod[(1 + i) * 64 + lane] = __dmul_rn(m, noise_blend(q, r, p, nr));
                    prod[(1 + N + i) * 64 + lane] = __dmul_rn(m, sc[i]);
                }
                prod[(1 + 2 * N) * 64 + lane] = __dmul_rn(m, noise_blend(q, price, p, a.noise_price[t]));
                if (a.pi) a.pi[g * J + k] = m;
            }
            __syncthreads();
            const int n = min(64, J - k0);
            acc = chain_read_back(prod, n_out, n, acc, lane);
            __syncthreads();
        }
        chain_store(a.iters, a.change, a.mass, a.stat_price, a.stat_reward, a.stat_action, g, G, N, lane, it, chg, acc);
        __syncthreads();                                 // this game's LDS reads before the next game's writes
    }
}

}  // namespace

int launch_stationary(const StatArgs& a, int grid, hipStream_t s) {
    if (a.cell_lds)
        hipLaunchKernelGGL((k_stationary<true>), dim3(grid), dim3(64), (size_t)a.lds_bytes, s, a);
    else
        hipLaunchKernelGGL((k_stationary<false>), dim3(grid), dim3(64), (size_t)a.lds_bytes, s, a);
    return (int)hipGetLastError();
}

}  // namespace thrl
