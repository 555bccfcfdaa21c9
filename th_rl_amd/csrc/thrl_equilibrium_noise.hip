// thrl_equilibrium_noise.hip -- the equilibrium check under demand noise (thrl_equilibrium_noise, include/thrl.h): per
// game and selected agent, policy iteration from the agent's own greedy strategy against the rivals' greedy strategies
// in the noisy environment, every evaluation a Jacobi iteration of the strategy's linear system on the price cells.
//
// One wavefront (a one-wave block) per game, looping over games, lanes owning cells k = lane, lane + 64, ...  Per game
// the wave gathers the tuple of every cell (k_stationary's gather); per agent it keeps in LDS both iterates, V_pi, the
// strategy, and per cell what a sweep needs of the strategy's tuple: its expected reward, deterministic successor and
// band place.  A sweep is then W + 1 LDS reads of V per cell and W band entries from the shared table in L2 (a lane
// walks its tuple's row, consecutive w at consecutive addresses); the wave reduces chg with __shfl_xor.  The improvement
// step needs z_V of every (cell, action): where the game has no more tuples than that and LDS has the room, z is staged
// once per tuple and round; otherwise it is computed per (cell, action).  z depends on the tuple alone, so both give the
// same bits.  The ordered output sums follow k_stationary: chunks of 64 cells, one lane per cell for the terms, then one
// lane per sum reading them back from LDS in ascending k (chain_read_back).
#include "thrl_equilibrium_noise.h"

#include "thrl_solve_dev.h"

namespace thrl {

namespace {

__global__ void __launch_bounds__(64) k_equilibrium_noise(const EqnArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    const int lane = threadIdx.x;
    const int N = a.N, G = a.G, J = a.J, W = a.W, TT = a.T;
    double* Va = reinterpret_cast<double*>(s_mem + a.o_va);
    double* Vb = reinterpret_cast<double*>(s_mem + a.o_vb);
    double* Vpi = reinterpret_cast<double*>(s_mem + a.o_vpi);
    double* Rs = reinterpret_cast<double*>(s_mem + a.o_rs);           // R(k, sigma(k))
    double* prod = reinterpret_cast<double*>(s_mem + a.o_prod);       // [kEqnSums][64] the chunk's terms per sum
    double* zt = reinterpret_cast<double*>(s_mem + a.o_zt);           // [T] z_V per tuple (zt_lds)
    int32_t* blo = reinterpret_cast<int32_t*>(s_mem + a.o_blo);       // band_lo of the cell's tuple under sigma
    uint32_t* tcur = reinterpret_cast<uint32_t*>(s_mem + a.o_tcur);   // that tuple: its band row
    uint16_t* sigma = reinterpret_cast<uint16_t*>(s_mem + a.o_sigma);
    uint16_t* base = reinterpret_cast<uint16_t*>(s_mem + a.o_base);   // the cell's tuple without agent i's action
    uint16_t* pol = reinterpret_cast<uint16_t*>(s_mem + a.o_pol);     // pi_i(k)
    uint16_t* tup = reinterpret_cast<uint16_t*>(s_mem + a.o_tup);
    uint16_t* det = reinterpret_cast<uint16_t*>(s_mem + a.o_det);     // det_cell of that tuple, 0xffff: no cell
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
        const uint16_t* __restrict__ pg = a.policy + g * a.P;
        const double p = a.noise_prob_g ? a.noise_prob_g[g] : a.noise_prob;
        const double q = __dsub_rn(1.0, p);
        if (!(p > 0.0 && p <= 1.0)) {                    // wave-uniform: no agent of this game is solved, zeros
            for (int i = 0; i < N; i++) {
                if (!((a.agents >> i) & 1)) continue;
                const int64_t o = (int64_t)i * G + g;
                if (lane == 0) {
                    a.iters[o] = -1; a.sweeps[o] = 0; a.n_diff_all[o] = 0;
                    a.loss_all[o] = 0.0; a.loss_all_mean[o] = 0.0;
                    if (a.weights) { a.loss_w[o] = 0.0; a.diff_w[o] = 0.0; a.v_w[o] = 0.0; }
                }
                store_states_unsolved(a, o * J, J, lane, 0.0, [](int) THRL_SOLVE_INLINE { return 0; });
            }
            continue;
        }

        // z_V(t) of the definition, V in LDS
        auto z_of = [&](const double* V, int t) -> double {
            const int d = a.det_cell[t];
            const int b0 = a.band_lo[t];
            const double* __restrict__ br = a.band + (int64_t)t * W;
            const double s0 = (d >= 0 && d < J) ? __dmul_rn(q, V[d]) : 0.0;
            double b = 0.0;
            for (int w = band_first(b0, W), we = band_end(b0, W, J); w < we; w++) b = __dadd_rn(b, __dmul_rn(br[w], V[b0 + w]));
            return __dadd_rn(s0, __dmul_rn(p, b));
        };

        // ---- the tuple of every cell
        for (int k = lane; k < J; k += 64) tup[k] = (uint16_t)cell_tuple(a, pg, a.cell_rows, J, k);
        __syncthreads();

        for (int i = 0; i < N; i++) {
            if (!((a.agents >> i) & 1)) continue;
            const int64_t o = (int64_t)i * G + g;
            const int nact = a.ag[i].n_actions, ts = a.tstride[i];
            const double gam = a.sweep_gamma ? a.sweep_gamma[o] : a.ag[i].gamma;
            const double* __restrict__ R = a.rew + (int64_t)i * TT;
            const double* __restrict__ NR = a.noise_reward + (int64_t)i * TT;
            auto reward = [&](int t) -> double { return noise_blend(q, R[t], p, NR[t]); };

            bool solved = gam >= 0.0 && gam < 1.0;       // wave-uniform throughout
            int iters = -1, sweeps = 0;
            double* V = Va;                              // the last iterate
            double* Vn = Vb;
            if (solved) {
                for (int k = lane; k < J; k += 64) {
                    const int t = tup[k];
                    const int ai = (t / ts) % nact;
                    pol[k] = (uint16_t)ai;
                    sigma[k] = (uint16_t)ai;
                    base[k] = (uint16_t)(t - ai * ts);
                    Va[k] = 0.0;
                }
                const double margin = improve_margin(gam, a.eval_tol);
                const bool staged = a.zt_lds && TT <= J * nact;
                __syncthreads();

                for (int n = 0;; n++) {
                    // ---- what a sweep needs of sigma's tuples
                    for (int k = lane; k < J; k += 64) {
                        const int t = (int)base[k] + (int)sigma[k] * ts;
                        const int d = a.det_cell[t];
                        Rs[k] = reward(t);
                        det[k] = (uint16_t)((d >= 0 && d < J) ? d : 0xffff);
                        blo[k] = a.band_lo[t];
                        tcur[k] = (uint32_t)t;
                    }
                    __syncthreads();

                    // ---- V = evaluation of sigma, from the V at hand
                    bool capped = false;
                    for (int m = 0;;) {
                        double c = 0.0;
                        for (int k = lane; k < J; k += 64) {
                            const int d = det[k];
                            const int b0 = blo[k];
                            const double* __restrict__ br = a.band + (int64_t)tcur[k] * W;
                            const double s0 = d != 0xffff ? __dmul_rn(q, V[d]) : 0.0;
                            double b = 0.0;
#pragma unroll 4
                            for (int w = band_first(b0, W), we = band_end(b0, W, J); w < we; w++)
                                b = __dadd_rn(b, __dmul_rn(br[w], V[b0 + w]));
                            const double v = __dadd_rn(Rs[k], __dmul_rn(gam, __dadd_rn(s0, __dmul_rn(p, b))));
                            Vn[k] = v;
                            c = fmax(c, fabs(__dsub_rn(v, V[k])));
                        }
#pragma unroll
                        for (int x = 32; x >= 1; x >>= 1) c = fmax(c, __shfl_xor(c, x));
                        __syncthreads();
                        double* tv = V; V = Vn; Vn = tv;
                        m++;
                        sweeps++;
                        if (c <= a.eval_tol) break;
                        if (m >= a.max_sweeps) { capped = true; break; }
                    }
                    if (capped) { solved = false; break; }
                    if (n == 0)
                        for (int k = lane; k < J; k += 64) Vpi[k] = V[k];
                    if (n == THRL_EQ_MAX_ITERS) { solved = false; break; }

                    // ---- improvement: keep the incumbent unless some action is better by more than the margin
                    if (staged) {
                        for (int t = lane; t < TT; t += 64) zt[t] = z_of(V, t);
                        __syncthreads();
                    }
                    bool changed = false;
                    for (int k = lane; k < J; k += 64) {
                        const int b = base[k], cur = sigma[k];
                        double bv, qc = 0.0;
                        const int ba = first_max(nact, [&](int act) THRL_SOLVE_INLINE {
                            const int t = b + act * ts;
                            const double z = staged ? zt[t] : z_of(V, t);
                            const double qv = __dadd_rn(reward(t), __dmul_rn(gam, z));
                            if (act == cur) qc = qv;
                            return qv;
                        }, bv);
                        if (bv > __dadd_rn(qc, margin)) { sigma[k] = (uint16_t)ba; changed = true; }
                    }
                    const bool any = __ballot(changed) != 0;
                    __syncthreads();                     // sigma of every lane; every read of V and zt before they change
                    if (!any) { iters = n; break; }
                }
            }
            __syncthreads();                             // Vpi and sigma of every lane

            if (!solved) {                               // a gamma outside [0, 1), or capped: NaN, br_policy = pi_i
                if (lane == 0) {
                    a.iters[o] = -1; a.sweeps[o] = sweeps; a.n_diff_all[o] = 0;
                    a.loss_all[o] = nan; a.loss_all_mean[o] = nan;
                    if (a.weights) { a.loss_w[o] = nan; a.diff_w[o] = nan; a.v_w[o] = nan; }
                }
                store_states_unsolved(a, o * J, J, lane, nan, [&](int k) THRL_SOLVE_INLINE { return ((int)tup[k] / ts) % nact; });
                __syncthreads();
                continue;
            }

            // ---- losses: per cell into the free V buffer, then the ordered sums
            double* loss = Vn;
            int nd = 0;
            double lmax = -__builtin_huge_val();
            for (int k = lane; k < J; k += 64) {
                const double vs = V[k], vp = Vpi[k];
                const double l = rel_loss(vs, vp);
                loss[k] = l;
                if (l > lmax) lmax = l;
                nd += sigma[k] != pol[k] ? 1 : 0;
                store_state(a, o * J + k, sigma[k], vs, vp);
            }
            wave_max_sum(lmax, nd);
            __syncthreads();
            const int n_sums = a.weights ? kEqnSums : 1;
            double acc = 0.0;
            for (int k0 = 0; k0 < J; k0 += 64) {
                const int k = k0 + lane;
                if (k < J) {
                    const double l = loss[k];
                    prod[lane] = l;
                    if (a.weights) {
                        const double w = a.weights[g * J + k];
                        prod[64 + lane] = __dmul_rn(w, l);
                        prod[128 + lane] = sigma[k] != pol[k] ? w : 0.0;
                        prod[192 + lane] = __dmul_rn(w, Vpi[k]);
                    }
                }
                __syncthreads();
                acc = chain_read_back(prod, n_sums, min(64, J - k0), acc, lane);
                __syncthreads();
            }
            if (lane == 0) {
                a.iters[o] = iters;
                a.sweeps[o] = sweeps;
                a.n_diff_all[o] = nd;
                a.loss_all[o] = lmax;
                a.loss_all_mean[o] = __ddiv_rn(acc, (double)J);
            } else if (a.weights && lane == 1) {
                a.loss_w[o] = acc;
            } else if (a.weights && lane == 2) {
                a.diff_w[o] = acc;
            } else if (a.weights && lane == 3) {
                a.v_w[o] = acc;
            }
            __syncthreads();                             // loss / V / sigma reads before the next agent's writes
        }
        __syncthreads();                                 // this game's LDS reads before the next game's writes
    }
}

}  // namespace

int launch_equilibrium_noise(const EqnArgs& a, int grid, hipStream_t s) {
    hipLaunchKernelGGL(k_equilibrium_noise, dim3(grid), dim3(64), (size_t)a.lds_bytes, s, a);
    return (int)hipGetLastError();
}

}  // namespace thrl
