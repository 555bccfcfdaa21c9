// thrl_tuple_equilibrium_noise.hip -- the equilibrium check under demand noise in tuple form
// (thrl_tuple_equilibrium_noise, include/thrl.h): per game and selected agent, policy iteration from the agent's own
// strategy against the rivals' strategies in the noisy environment, on the S = T + J states "the price is exactly tuple
// t's" and "the price lies in cell k", every evaluation a Jacobi iteration of the strategy's linear system.
//
// One wavefront (a one-wave block) per game, looping over games.  Both the expected reward and the continuation value
// of a state depend on the tuple played there alone, and there are fewer tuples than states, so a sweep has two
// phases: lanes owning tuples t = lane, lane + 64, ... compute x(t) = R(t) + gamma * z_V(t) into LDS (the only walk over
// a band row: W band entries from the shared table in L2, consecutive w at consecutive addresses, and W + 1 LDS reads
// of V), then lanes owning states read V'(s) = x(t(s, sigma(s))) back and the wave reduces chg with __shfl_xor.  The
// improvement step reads the same array, computed once more from the last iterate: Q(s, a) = x(t(s, a)).  Per game the
// wave keeps the tuple every state plays; per agent both iterates, V_pi, x, R per tuple and the current strategy's
// tuple per state; the actions are recovered from the tuples by division where a round ends.  The ordered output sums
// follow k_equilibrium_noise: chunks of 64 states (the tuple-states, then the cells), one lane per state for the
// terms, then one lane per sum reading them back from LDS in ascending order.
#include "thrl_tuple_equilibrium_noise.h"

#include "thrl_solve_dev.h"

namespace thrl {

namespace {

typedef double band4 __attribute__((ext_vector_type(4), aligned(8)));    // four band entries of a row, one load

__global__ void __launch_bounds__(64) k_tuple_equilibrium_noise(const TenArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    const int lane = threadIdx.x;
    const int N = a.N, G = a.G, T = a.T, J = a.J, W = a.W, S = a.T + a.J;
    double* Va = reinterpret_cast<double*>(s_mem + a.o_va);
    double* Vb = reinterpret_cast<double*>(s_mem + a.o_vb);
    double* Vpi = reinterpret_cast<double*>(s_mem + a.o_vpi);
    double* xt = reinterpret_cast<double*>(s_mem + a.o_x);            // [T] R(t) + gamma * z_V(t)
    double* Rt = reinterpret_cast<double*>(s_mem + a.o_rt);           // [T] R(t) of this agent and game
    double* prod = reinterpret_cast<double*>(s_mem + a.o_prod);       // [kTenSums][64] the chunk's terms per sum
    uint16_t* tup = reinterpret_cast<uint16_t*>(s_mem + a.o_tup);     // [S] the tuple played at the state
    uint16_t* tcur = reinterpret_cast<uint16_t*>(s_mem + a.o_tcur);   // [S] t(s, sigma(s))
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
        const double p = a.noise_prob_g ? a.noise_prob_g[g] : a.noise_prob;
        const double q = __dsub_rn(1.0, p);
        if (!(p > 0.0 && p <= 1.0)) {                    // wave-uniform: no agent of this game is solved, zeros
            for (int i = 0; i < N; i++) {
                if (!((a.agents >> i) & 1)) continue;
                const int64_t o = (int64_t)i * G + g;
                if (lane == 0) {
                    a.iters[o] = -1; a.sweeps[o] = 0; a.n_diff_tuples[o] = 0; a.n_diff_cells[o] = 0;
                    a.loss_all[o] = 0.0; a.loss_tuples_mean[o] = 0.0; a.loss_cells_mean[o] = 0.0;
                    if (a.pi) { a.loss_w[o] = 0.0; a.diff_w[o] = 0.0; a.v_w[o] = 0.0; }
                }
                store_states_unsolved(a, o * S, S, lane, 0.0, [](int) THRL_SOLVE_INLINE { return 0; });
            }
            continue;
        }

        // ---- the tuple of every state: F_g(t) at the tuple-states, tau_g(k) at the cells
        const uint16_t* __restrict__ tp = a.tuple_policy + g * N * T;
        const uint16_t* __restrict__ cp = a.cell_policy + g * N * J;
        for (int s = lane; s < S; s += 64) {
            int t = 0;
            for (int i = 0; i < N; i++) {
                const int e = s < T ? (int)tp[(int64_t)i * T + s] : (int)cp[(int64_t)i * J + (s - T)];
                t += min(e, a.n_actions[i] - 1) * a.tstride[i];
            }
            tup[s] = (uint16_t)t;
        }
        __syncthreads();

        for (int i = 0; i < N; i++) {
            if (!((a.agents >> i) & 1)) continue;
            const int64_t o = (int64_t)i * G + g;
            const int nact = a.n_actions[i], ts = a.tstride[i];
            const double gam = a.sweep_gamma ? a.sweep_gamma[o] : a.gamma[i];

            // x(t) = R(t) + gamma * z_V(t) of every tuple, V in LDS; the cells of a band row that lie in [0, J) are
            // [w0, w1), at most J of them whatever W and band_lo are
            auto stage_x = [&](const double* V) {
                const double* VJ = V + T;
                for (int t = lane; t < T; t += 64) {
                    const int b0 = a.band_lo[t];
                    const double* __restrict__ br = a.band + (int64_t)t * W;
                    const int w0 = band_first(b0, W), w1 = band_end(b0, W, J);
                    // every lane walks a row of its own, so a load touches 64 cache lines whatever its width: four
                    // entries per load (8-byte aligned: W may be odd), the adds in the order of the definition
                    double b = 0.0;
                    int w = w0;
#pragma unroll 2
                    for (; w + 4 <= w1; w += 4) {
                        const band4 n4 = *reinterpret_cast<const band4*>(br + w);
                        const double* v = VJ + b0 + w;
                        b = __dadd_rn(b, __dmul_rn(n4.x, v[0]));
                        b = __dadd_rn(b, __dmul_rn(n4.y, v[1]));
                        b = __dadd_rn(b, __dmul_rn(n4.z, v[2]));
                        b = __dadd_rn(b, __dmul_rn(n4.w, v[3]));
                    }
                    for (; w < w1; w++) b = __dadd_rn(b, __dmul_rn(br[w], VJ[b0 + w]));
                    const double z = __dadd_rn(__dmul_rn(q, V[t]), __dmul_rn(p, b));
                    xt[t] = __dadd_rn(Rt[t], __dmul_rn(gam, z));
                }
            };

            bool solved = gam >= 0.0 && gam < 1.0;       // wave-uniform throughout
            int iters = -1, sweeps = 0;
            double* V = Va;                              // the last iterate
            double* Vn = Vb;
            if (solved) {
                for (int s = lane; s < S; s += 64) {
                    tcur[s] = tup[s];
                    Va[s] = 0.0;
                }
                for (int t = lane; t < T; t += 64)
                    Rt[t] = noise_blend(q, a.reward[(int64_t)i * T + t], p, a.noise_reward[(int64_t)i * T + t]);
                const double margin = improve_margin(gam, a.eval_tol);
                __syncthreads();

                for (int n = 0;; n++) {
                    // ---- V = evaluation of sigma, from the V at hand
                    bool capped = false;
                    for (int m = 0;;) {
                        stage_x(V);
                        __syncthreads();
                        double c = 0.0;
                        for (int s = lane; s < S; s += 64) {
                            const double v = xt[tcur[s]];
                            Vn[s] = v;
                            c = fmax(c, fabs(__dsub_rn(v, V[s])));
                        }
#pragma unroll
                        for (int x = 32; x >= 1; x >>= 1) c = fmax(c, __shfl_xor(c, x));
                        __syncthreads();                 // Vn of every lane; every read of xt and V before they change
                        double* tv = V; V = Vn; Vn = tv;
                        m++;
                        sweeps++;
                        if (c <= a.eval_tol) break;
                        if (m >= a.max_sweeps) { capped = true; break; }
                    }
                    if (capped) { solved = false; break; }
                    if (n == 0)
                        for (int s = lane; s < S; s += 64) Vpi[s] = V[s];
                    if (n == THRL_EQ_MAX_ITERS) { solved = false; break; }

                    // ---- improvement: keep the incumbent unless some action is better by more than the margin
                    stage_x(V);
                    __syncthreads();
                    bool changed = false;
                    for (int s = lane; s < S; s += 64) {
                        const int t0 = tup[s], tc = tcur[s];
                        const int b = t0 - ((t0 / ts) % nact) * ts;
                        const double qc = xt[tc];
                        double bv;
                        const int ba = first_max(nact, [&](int act) THRL_SOLVE_INLINE { return xt[b + act * ts]; }, bv);
                        if (bv > __dadd_rn(qc, margin)) { tcur[s] = (uint16_t)(b + ba * ts); changed = true; }
                    }
                    const bool any = __ballot(changed) != 0;
                    __syncthreads();                     // tcur of every lane; every read of xt before it changes
                    if (!any) { iters = n; break; }
                }
            }
            __syncthreads();                             // Vpi and tcur of every lane

            if (!solved) {                               // a gamma outside [0, 1), or capped: NaN, br_policy = pi_i
                if (lane == 0) {
                    a.iters[o] = -1; a.sweeps[o] = sweeps; a.n_diff_tuples[o] = 0; a.n_diff_cells[o] = 0;
                    a.loss_all[o] = nan; a.loss_tuples_mean[o] = nan; a.loss_cells_mean[o] = nan;
                    if (a.pi) { a.loss_w[o] = nan; a.diff_w[o] = nan; a.v_w[o] = nan; }
                }
                store_states_unsolved(a, o * S, S, lane, nan, [&](int s) THRL_SOLVE_INLINE { return ((int)tup[s] / ts) % nact; });
                __syncthreads();
                continue;
            }

            // ---- losses: per state into the free V buffer, then the ordered sums
            double* loss = Vn;
            int ndt = 0, ndc = 0;
            double lmax = -__builtin_huge_val();
            for (int s = lane; s < S; s += 64) {
                const double vs = V[s], vp = Vpi[s];
                const double l = rel_loss(vs, vp);
                loss[s] = l;
                if (l > lmax) lmax = l;
                const int d = tcur[s] != tup[s] ? 1 : 0;
                if (s < T) ndt += d; else ndc += d;
                store_state(a, o * S + s, ((int)tcur[s] / ts) % nact, vs, vp);
            }
            // two counts in one loop, not wave_max_sum and a second loop: that order of the shuffles costs 68 bytes of scratch
#pragma unroll
            for (int x = 32; x >= 1; x >>= 1) {
                const double ol = __shfl_xor(lmax, x);
                if (ol > lmax) lmax = ol;
                ndt += __shfl_xor(ndt, x);
                ndc += __shfl_xor(ndc, x);
            }
            __syncthreads();
            // lane 0: the loss over the tuple-states, lane 1: over the cells, lanes 2..4: the weighted sums over both
            const double* __restrict__ pig = a.pi ? a.pi + g * T : nullptr;
            double acc = 0.0;
            for (int seg = 0; seg < 2; seg++) {
                const int s_lo = seg == 0 ? 0 : T, s_hi = seg == 0 ? T : S;
                for (int s0 = s_lo; s0 < s_hi; s0 += 64) {
                    const int s = s0 + lane;
                    if (s < s_hi) {
                        const double l = loss[s];
                        prod[lane] = l;
                        if (pig) {
                            double w;
                            if (seg == 0) {
                                w = __dmul_rn(q, pig[s]);
                            } else {                     // nu(k): the long-run mass a shock puts into cell k
                                const int k = s - T;
                                double nu = 0.0;
                                for (int t = 0; t < T; t++) {
                                    const uint32_t d = (uint32_t)(k - a.band_lo[t]);
                                    if (d < (uint32_t)W) nu = __dadd_rn(nu, __dmul_rn(pig[t], a.band[(int64_t)t * W + d]));
                                }
                                w = __dmul_rn(p, nu);
                            }
                            prod[64 + lane] = __dmul_rn(w, l);
                            prod[128 + lane] = tcur[s] != tup[s] ? w : 0.0;
                            prod[192 + lane] = __dmul_rn(w, Vpi[s]);
                        }
                    }
                    __syncthreads();
                    const int cnt = min(64, s_hi - s0);
                    if (lane == seg || (pig && lane >= 2 && lane < 2 + kTenSums - 1)) {
                        const double* pr = prod + (lane < 2 ? 0 : lane - 1) * 64;
                        for (int kk = 0; kk < cnt; kk++) acc = __dadd_rn(acc, pr[kk]);
                    }
                    __syncthreads();
                }
            }
            if (lane == 0) {
                a.iters[o] = iters;
                a.sweeps[o] = sweeps;
                a.n_diff_tuples[o] = ndt;
                a.n_diff_cells[o] = ndc;
                a.loss_all[o] = lmax;
                a.loss_tuples_mean[o] = __ddiv_rn(acc, (double)T);
            } else if (lane == 1) {
                a.loss_cells_mean[o] = __ddiv_rn(acc, (double)J);
            } else if (pig && lane == 2) {
                a.loss_w[o] = acc;
            } else if (pig && lane == 3) {
                a.diff_w[o] = acc;
            } else if (pig && lane == 4) {
                a.v_w[o] = acc;
            }
            __syncthreads();                             // loss / V / tcur reads before the next agent's writes
        }
        __syncthreads();                                 // this game's LDS reads before the next game's writes
    }
}

}  // namespace

int launch_tuple_equilibrium_noise(const TenArgs& a, int grid, hipStream_t s) {
    if (a.lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_tuple_equilibrium_noise),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, a.lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k_tuple_equilibrium_noise, dim3(grid), dim3(64), (size_t)a.lds_bytes, s, a);
    return (int)hipGetLastError();
}

}  // namespace thrl
