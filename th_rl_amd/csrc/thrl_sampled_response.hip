// thrl_sampled_response.hip -- exact best responses to the rivals' STOCHASTIC policies (thrl_sampled_response,
// include/thrl_response.h): per game and selected agent, the value V_pi of the agent's own mixed policy against the
// sampling rivals, and V*, sigma* by policy iteration over deterministic strategies, on the D distinct prices.  One kernel.
//
// k_sr_response: a 256-thread block per game, looping over games and the selected agents.  Per game the block stages the
//   rows at the distinct prices exactly as k_sp_chain does (sp_stage_game); per agent it keeps Z_-i(d) and S_i(d), the
//   agent's rewards R(t), both iterates, V_pi, the strategy and the modal action, and per sweep U(t) = R(t) + gamma
//   V(row(t)), rebuilt once.  Q_V(d, k) is an ordered sum over the T / A_i tuples in which the agent plays k: no split of
//   it, no matrix instruction.  A sweep of the mixed policy and an improvement step need every Q_V(d, k): a thread owns a
//   price and walks k ascending, or, where there are fewer than 129 prices, a team of threads shares a price's actions
//   through a staging array and the team's first thread adds them up in order.  A sweep of a deterministic strategy needs
//   one Q_V(d, sigma(d)) per price: a thread per price, 1 / A_i of the work.  The largest change is a maximum, whose
//   order is free: sp_block_max.  The ordered output sums are one lane each over the D terms.
//   Here are the sweeps and the improvement step with their team split, the agent's rewards and the weights M(d).  The
//   game's staging and the block maximum are thrl_sampled_dev.h's; the margin, the first maximum and the relative loss
//   are thrl_solve_dev.h's; sr_prob and sr_q, the staging of the grouping, the outputs of a refused game and of an
//   unsolved agent, the per-price setup, a solved price's stores, the loss sums and the four weighted sums are
//   thrl_response_dev.h's, shared with k_srn_response; the launch is thrl_sampled.h's sp_launch.
//   Nothing in the body is wave-specific: with THRL_SP_HOST_BUILD the same source runs as 256 host threads with barriers.
#include "thrl_response_dev.h"

namespace thrl {

namespace {

template <int MAXN>
__device__ __forceinline__ void sr_block(const SrArgs& a, unsigned char* s_mem, int tid, int bid, int nblk) {
    const SpArgs& sp = a.sp;
    const int N = sp.N, G = sp.G, T = sp.T, D = sp.D, team = a.team;
    double* Va = reinterpret_cast<double*>(s_mem + a.o_va);
    double* Vb = reinterpret_cast<double*>(s_mem + a.o_vb);
    double* Vpi = reinterpret_cast<double*>(s_mem + a.o_vpi);
    double* Zm = reinterpret_cast<double*>(s_mem + a.o_zm);           // [D] Z_-i(d)
    double* Si = reinterpret_cast<double*>(s_mem + a.o_si);           // [D] S_i(d)
    double* U = reinterpret_cast<double*>(s_mem + a.o_u);             // [T] R(t) + gamma V(row(t)); M(d) for the outputs
    double* Rt = reinterpret_cast<double*>(s_mem + a.o_rt);           // [T] reward_i(t)
    double* Qs = reinterpret_cast<double*>(s_mem + a.o_q);            // [D][A_i] with team > 1
    uint16_t* first = reinterpret_cast<uint16_t*>(s_mem + sp.o_first);
    uint16_t* perm = reinterpret_cast<uint16_t*>(s_mem + sp.o_perm);
    uint16_t* trow = reinterpret_cast<uint16_t*>(s_mem + a.o_trow);   // [T] row(t)
    uint16_t* sigma = reinterpret_cast<uint16_t*>(s_mem + a.o_sigma);
    uint16_t* modal = reinterpret_cast<uint16_t*>(s_mem + a.o_modal);
    double* prod = reinterpret_cast<double*>(s_mem + sp.o_prod);      // [256] the threads' maxima
    SpCst* cst = reinterpret_cast<SpCst*>(s_mem + sp.o_cst);

    sr_stage_grouping(sp, first, perm, trow, tid);       // per config, staged once

    for (int64_t g = bid; g < G; g += nblk) {
        if (!sp_eps_ok(sp, g)) {                         // block-uniform: no agent of this game is solved, zeros
            for (int i = 0; i < N; i++)
                if ((a.agents >> i) & 1) sr_flat_outputs(a, (int64_t)i * G + g, D, 0.0, 0, nullptr, tid);
            continue;
        }
        __syncthreads();                                 // the game before is read to its end; the grouping is staged

        // ---- the game's rows and constants
        sp_stage_game<1>(sp, s_mem, cst, g, tid);
        __syncthreads();

        for (int i = 0; i < N; i++) {
            if (!((a.agents >> i) & 1)) continue;
            const int64_t o = (int64_t)i * G + g;
            const int A = sp.n_actions[i];
            const double gam = a.sweep_gamma ? a.sweep_gamma[o] : a.gamma[i];

            // ---- per price: Z_-i, S_i and the modal action; per tuple: the agent's reward
            sr_setup_states(sp, i, D, Zm, Si, modal, sigma, Va, tid,
                            [&](int j, int d, int k) THRL_SOLVE_INLINE { return sr_prob(sp, s_mem, cst, j, d, k); },
                            [&](int d) THRL_SOLVE_INLINE { return (int)reinterpret_cast<const uint16_t*>(s_mem + sp.o_row[i])[d]; });
            for (int t = tid; t < T; t += kSpBlock) Rt[t] = sp.reward[(int64_t)i * T + t];

            double* V = Va;                              // the last iterate
            double* Vn = Vb;
            int sweeps = 0;

            // Jacobi sweeps of V' = the mixed policy's (mixed) or sigma's value from V until chg <= eval_tol; true: capped
            auto evaluate = [&](bool mixed) THRL_SOLVE_INLINE {
                for (int m = 0;;) {
                    __syncthreads();                     // V of every thread; the reads of U before it changes
                    for (int t = tid; t < T; t += kSpBlock) U[t] = __dadd_rn(Rt[t], __dmul_rn(gam, V[trow[t]]));
                    __syncthreads();
                    double c = 0.0;
                    if (!mixed) {
                        for (int d = tid; d < D; d += kSpBlock) {
                            const double v = sr_q<MAXN>(sp, s_mem, cst, U, Zm[d], i, d, sigma[d]);
                            Vn[d] = v;
                            c = fmax(c, fabs(__dsub_rn(v, V[d])));
                        }
                    } else if (team == 1) {
                        for (int d = tid; d < D; d += kSpBlock) {
                            double s = 0.0;
                            for (int k = 0; k < A; k++)
                                s = __dadd_rn(s, __dmul_rn(sr_prob(sp, s_mem, cst, i, d, k), sr_q<MAXN>(sp, s_mem, cst, U, Zm[d], i, d, k)));
                            const double v = __ddiv_rn(s, Si[d]);
                            Vn[d] = v;
                            c = fmax(c, fabs(__dsub_rn(v, V[d])));
                        }
                    } else {
                        const int d = tid / team;
                        if (d < D)
                            for (int k = tid % team; k < A; k += team) Qs[d * A + k] = sr_q<MAXN>(sp, s_mem, cst, U, Zm[d], i, d, k);
                        __syncthreads();
                        if (tid < D) {
                            double s = 0.0;
                            for (int k = 0; k < A; k++) s = __dadd_rn(s, __dmul_rn(sr_prob(sp, s_mem, cst, i, tid, k), Qs[tid * A + k]));
                            const double v = __ddiv_rn(s, Si[tid]);
                            Vn[tid] = v;
                            c = fmax(c, fabs(__dsub_rn(v, V[tid])));
                        }
                    }
                    c = sp_block_max(prod, cst, c, tid);
                    double* tv = V; V = Vn; Vn = tv;
                    m++;
                    sweeps++;
                    if (c <= a.eval_tol) return false;
                    if (m >= a.max_sweeps) return true;
                }
            };

            bool solved = gam >= 0.0 && gam < 1.0;       // block-uniform throughout
            int iters = -1;
            if (solved) {
                // ---- V_pi: the agent's own mixed policy, from 0
                if (evaluate(true)) solved = false;
            }
            if (solved) {
                __syncthreads();
                for (int d = tid; d < D; d += kSpBlock) Vpi[d] = V[d];
                const double margin = improve_margin(gam, a.eval_tol);
                for (int n = 0;; n++) {
                    // ---- V = evaluation of sigma, from the V at hand (round 0: from V_pi)
                    if (evaluate(false)) { solved = false; break; }
                    if (n == THRL_EQ_MAX_ITERS) { solved = false; break; }

                    // ---- improvement: keep the incumbent unless some action is better by more than the margin
                    __syncthreads();
                    for (int t = tid; t < T; t += kSpBlock) U[t] = __dadd_rn(Rt[t], __dmul_rn(gam, V[trow[t]]));
                    __syncthreads();
                    bool changed = false;
                    if (team == 1) {
                        for (int d = tid; d < D; d += kSpBlock) {
                            const double qc = sr_q<MAXN>(sp, s_mem, cst, U, Zm[d], i, d, sigma[d]);
                            double bv;
                            const int ba = first_max(A, [&](int k) THRL_SOLVE_INLINE { return sr_q<MAXN>(sp, s_mem, cst, U, Zm[d], i, d, k); }, bv);
                            if (bv > __dadd_rn(qc, margin)) { sigma[d] = (uint16_t)ba; changed = true; }
                        }
                    } else {
                        const int d = tid / team;
                        if (d < D)
                            for (int k = tid % team; k < A; k += team) Qs[d * A + k] = sr_q<MAXN>(sp, s_mem, cst, U, Zm[d], i, d, k);
                        __syncthreads();
                        if (tid < D) {
                            const double qc = Qs[tid * A + sigma[tid]];
                            double bv;
                            const int ba = first_max(A, [&](int k) THRL_SOLVE_INLINE { return Qs[tid * A + k]; }, bv);
                            if (bv > __dadd_rn(qc, margin)) { sigma[tid] = (uint16_t)ba; changed = true; }
                        }
                    }
                    const bool any = sp_block_max(prod, cst, changed ? 1.0 : 0.0, tid) > 0.0;
                    if (!any) { iters = n; break; }
                }
            }
            __syncthreads();                             // Vpi, V and sigma of every thread

            if (!solved) {                               // a gamma outside [0, 1), or capped: NaN, br_policy = the modal action
                sr_flat_outputs(a, o, D, __builtin_nan(""), sweeps, modal, tid);
                __syncthreads();
                continue;
            }

            // ---- losses per price into the free V buffer, M(d) into U, then the ordered sums: one lane each
            double* loss = Vn;
            const double* __restrict__ pig = a.pi ? a.pi + g * T : nullptr;
            for (int d = tid; d < D; d += kSpBlock) {
                sr_store_state(a, o, D, d, V, Vpi, sigma, loss);
                if (pig) {
                    double M = 0.0;
                    const int e = first[d + 1];
                    for (int s = first[d]; s < e; s++) M = __dadd_rn(M, pig[perm[s]]);
                    U[d] = M;
                }
            }
            __syncthreads();
            if (tid == 0) {
                double lmax = -__builtin_huge_val(), acc = 0.0;
                int nd = 0;
                sr_loss_range(loss, sigma, modal, 0, D, lmax, acc, nd);
                a.iters[o] = iters; a.sweeps[o] = sweeps;
                sr_summary(a, o, lmax, nd, acc, 0, 0.0);
            } else if (pig) {                            // the weights M(d) are in U
                sr_weighted_sums(a, o, D, U, loss, V, Vpi, Si, sigma, tid,
                                 [&](int d, int k) THRL_SOLVE_INLINE { return sr_prob(sp, s_mem, cst, i, d, k); });
            }
            __syncthreads();                             // loss / V / sigma reads before the next agent's writes
        }
    }
}

#ifndef THRL_SP_HOST_BUILD
template <int MAXN>
__global__ void __launch_bounds__(kSpBlock) k_sr_response(const SrArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    sr_block<MAXN>(a, s_mem, (int)threadIdx.x, (int)blockIdx.x, (int)gridDim.x);
}
#endif

}  // namespace

#ifndef THRL_SP_HOST_BUILD
int launch_sampled_response(const SrArgs& a, int grid, hipStream_t s) {
    return sp_launch(k_sr_response<2>, k_sr_response<kSpMaxA>, a, a.sp, grid, s);
}
#endif

}  // namespace thrl
