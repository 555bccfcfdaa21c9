// thrl_sampled_response_noise.hip -- exact best responses to the rivals' STOCHASTIC policies UNDER DEMAND NOISE
// (thrl_sampled_response_noise, include/thrl_response_noise.h): thrl_sampled_response's problem in the environment of
// thrl_sampled_noise_chain.  An agent sees the price, so its states are the D distinct prices (reached with probability q
// after a tuple) and then the Jn quadrature nodes of the redrawn price, S = D + Jn in all.  One kernel.
//
// k_srn_response: a 256-thread block per game, looping over games and the selected agents, in k_sr_response's shape.  Per
//   game the block stages the rows at the distinct prices (sp_stage_game) and the QTable agents' node entries; per agent
//   it keeps Z_-i(s) and S_i(s) over the S states, Rn(t) = q reward + p noise_reward, both iterates, V_pi, the strategy
//   and the modal action.  A sweep first rebuilds U(t) = Rn(t) + gamma (q V_D(row(t)) + p b_V(t)) once per tuple, a
//   thread per tuple walking its band row in ascending node (band from global memory: it is per config and the games of
//   a grid share it through the caches), then a thread per state takes Q_V(s, .) from U: sr_q's ordered sum (sr_q_of)
//   with the state's probabilities, a price's or a node's.  A QTable rival's node row is an entry in LDS; a network's
//   node rows (4 Jn A_j bytes, more than the rest of the working set) stay in global memory and are read every sweep:
//   the threads of a wave own adjacent nodes, whose rows are adjacent.  The largest change is a maximum over all S
//   states (sp_block_max).  The ordered output sums are one lane each over the S terms, prices first.
//   Here are a state's probabilities (a price's or a node's), the one loop of the sweeps with its band walk, the agent's
//   rewards under noise and the weights w(s).  The game's staging and the block maximum are thrl_sampled_dev.h's; the
//   margin, the relative loss and the band's limits thrl_solve_dev.h's; sr_prob / sr_q / sr_q_of, the staging of the
//   grouping, the outputs of a refused game and of an unsolved agent, the per-state setup, a solved state's stores, the
//   loss sums and the four weighted sums are thrl_response_dev.h's, shared with k_sr_response; the launch is
//   thrl_sampled.h's sp_launch.  Nothing in the body is wave-specific: with THRL_SP_HOST_BUILD the same source runs as
//   256 host threads with barriers.
#include "thrl_response_dev.h"

namespace thrl {

namespace {

// A network's node rows as the global memory they are: a load through this type and a load from the staged rows are
// never merged into one load through a generic pointer
#ifdef THRL_SP_HOST_BUILD
typedef const float* SrnGlobalFloats;
#else
typedef const __attribute__((address_space(1))) float* SrnGlobalFloats;
#endif

// Pn_j(x|n) at node n of game g: a QTable agent's from its staged entry, a network's from global memory
__device__ __forceinline__ double srn_node_prob(const SrnArgs& a, const unsigned char* s_mem, const SpCst* cst, int64_t g, int j,
                                                int n, int x) {
    if (a.sp.kind[j] == 0) {
        const uint16_t* rq = reinterpret_cast<const uint16_t*>(s_mem + a.o_nrow[j]);
        return (int)rq[n] == x ? cst->hi[j] : cst->lo[j];
    }
    return (double)((SrnGlobalFloats)a.nprob[j])[(g * a.Jn + n) * a.sp.n_actions[j] + x];
}

// P_j(x|s) at state s: the price s below D, else the node s - D
__device__ __forceinline__ double srn_prob(const SrnArgs& a, const unsigned char* s_mem, const SpCst* cst, int64_t g, int j, int s,
                                           int x) {
    return s < a.sp.D ? sr_prob(a.sp, s_mem, cst, j, s, x) : srn_node_prob(a, s_mem, cst, g, j, s - a.sp.D, x);
}

// Q_V(s, k) of agent i at state s of game g: the kind of state is decided once, outside the walk over the state's tuples
template <int MAXN>
__device__ __forceinline__ double srn_q(const SrnArgs& a, const unsigned char* s_mem, const SpCst* cst, const double* U, double zm,
                                        int64_t g, int i, int s, int k) {
    if (s < a.sp.D) return sr_q<MAXN>(a.sp, s_mem, cst, U, zm, i, s, k);
    const int n = s - a.sp.D;
    return sr_q_of<MAXN>(a.sp, U, zm, i, k, [&](int j, int x) THRL_SOLVE_INLINE { return srn_node_prob(a, s_mem, cst, g, j, n, x); });
}

template <int MAXN>
__device__ __forceinline__ void srn_block(const SrnArgs& a, unsigned char* s_mem, int tid, int bid, int nblk) {
    const SpArgs& sp = a.sp;
    const int N = sp.N, G = sp.G, T = sp.T, D = sp.D, Jn = a.Jn, W = a.W, S = D + Jn;
    double* Va = reinterpret_cast<double*>(s_mem + a.o_va);           // [S]: the prices' values, then the nodes'
    double* Vb = reinterpret_cast<double*>(s_mem + a.o_vb);
    double* Vpi = reinterpret_cast<double*>(s_mem + a.o_vpi);
    double* Zm = reinterpret_cast<double*>(s_mem + a.o_zm);           // [S] Z_-i(s); the weights w(s) for the outputs
    double* Si = reinterpret_cast<double*>(s_mem + a.o_si);           // [S] S_i(s)
    double* U = reinterpret_cast<double*>(s_mem + a.o_u);             // [T] U_V(t)
    double* Rt = reinterpret_cast<double*>(s_mem + a.o_rt);           // [T] Rn(t)
    uint16_t* first = reinterpret_cast<uint16_t*>(s_mem + sp.o_first);
    uint16_t* perm = reinterpret_cast<uint16_t*>(s_mem + sp.o_perm);
    uint16_t* trow = reinterpret_cast<uint16_t*>(s_mem + a.o_trow);   // [T] row(t)
    uint16_t* sigma = reinterpret_cast<uint16_t*>(s_mem + a.o_sigma); // [S]
    uint16_t* modal = reinterpret_cast<uint16_t*>(s_mem + a.o_modal); // [S]
    double* prod = reinterpret_cast<double*>(s_mem + sp.o_prod);      // [256] the threads' maxima
    SpCst* cst = reinterpret_cast<SpCst*>(s_mem + sp.o_cst);

    sr_stage_grouping(sp, first, perm, trow, tid);       // per config, staged once

    for (int64_t g = bid; g < G; g += nblk) {
        const double p = a.noise_prob_g ? a.noise_prob_g[g] : a.noise_prob;
        if (!(sp_eps_ok(sp, g) && p > 0.0 && p <= 1.0)) { // block-uniform: no agent of this game is solved, zeros
            for (int i = 0; i < N; i++)
                if ((a.agents >> i) & 1) sr_flat_outputs(a, (int64_t)i * G + g, S, 0.0, 0, nullptr, tid);
            continue;
        }
        const double q = __dsub_rn(1.0, p);
        __syncthreads();                                 // the game before is read to its end; the grouping is staged

        // ---- the game's rows and constants, and the QTable agents' entries at the nodes
        sp_stage_game<1>(sp, s_mem, cst, g, tid);
        for (int i = 0; i < N; i++) {
            if (sp.kind[i] != 0) continue;
            uint16_t* rq = reinterpret_cast<uint16_t*>(s_mem + a.o_nrow[i]);
            const uint16_t* __restrict__ src = a.npolicy + (g * N + i) * Jn;
            const int A = sp.n_actions[i];
            for (int n = tid; n < Jn; n += kSpBlock) rq[n] = (uint16_t)min((int)src[n], A - 1);
        }
        __syncthreads();

        for (int i = 0; i < N; i++) {
            if (!((a.agents >> i) & 1)) continue;
            const int64_t o = (int64_t)i * G + g;
            const int A = sp.n_actions[i];
            const double gam = a.sweep_gamma ? a.sweep_gamma[o] : a.gamma[i];

            // ---- per state: Z_-i, S_i and the modal action; per tuple: the agent's reward under noise
            sr_setup_states(sp, i, S, Zm, Si, modal, sigma, Va, tid,
                            [&](int j, int s, int k) THRL_SOLVE_INLINE { return srn_prob(a, s_mem, cst, g, j, s, k); },
                            [&](int s) THRL_SOLVE_INLINE {
                                return (int)(s < D ? reinterpret_cast<const uint16_t*>(s_mem + sp.o_row[i])[s]
                                                   : reinterpret_cast<const uint16_t*>(s_mem + a.o_nrow[i])[s - D]);
                            });
            for (int t = tid; t < T; t += kSpBlock)
                Rt[t] = __dadd_rn(__dmul_rn(q, sp.reward[(int64_t)i * T + t]), __dmul_rn(p, a.noise_reward[(int64_t)i * T + t]));

            double* V = Va;                              // the last iterate
            double* Vn = Vb;
            int sweeps = 0;
            bool solved = gam >= 0.0 && gam < 1.0;       // block-uniform throughout
            int iters = -1;
            const double margin = improve_margin(gam, a.eval_tol);

            // One loop serves the three passes over the states, so that the block's code holds one copy of the band walk and
            // of the walks over a state's tuples.  kMixed: Jacobi sweeps of the agent's own mixed policy from 0 until chg <=
            // eval_tol (V_pi); kSigma: the same of sigma, from the V at hand; kImprove: keep the incumbent unless some
            // action is better by more than the margin.  m counts the sweeps of the evaluation at hand, n the rounds.
            enum { kMixed, kSigma, kImprove };
            for (int mode = kMixed, m = 0, n = 0; solved;) {
                __syncthreads();                         // V of every thread; the reads of U before it changes
                // U_V(t) = Rn(t) + gamma (q V_D(row(t)) + p b_V(t)), b_V the band row's ordered sum over the nodes in [0, Jn)
                {
                    const double* VN = V + D;
                    for (int t = tid; t < T; t += kSpBlock) {
                        const int b0 = a.band_lo[t];
                        const double* __restrict__ bt = a.band + (int64_t)t * W;
                        const int we = band_end(b0, W, Jn);
                        double b = 0.0;
                        // (eight loads in flight ahead of the chain of additions: a rolled loop waits for memory per node)
#pragma unroll 8
                        for (int w = band_first(b0, W); w < we; w++) b = __dadd_rn(b, __dmul_rn(bt[w], VN[b0 + w]));
                        const double z = __dadd_rn(__dmul_rn(q, V[trow[t]]), __dmul_rn(p, b));
                        U[t] = __dadd_rn(Rt[t], __dmul_rn(gam, z));
                    }
                }
                __syncthreads();
                double c = 0.0;                          // the largest change; kImprove: 1.0 where a state changed
                for (int s = tid; s < S; s += kSpBlock) {
                    const int sg = sigma[s];
                    const double zm = Zm[s];
                    if (mode == kSigma) {
                        const double v = srn_q<MAXN>(a, s_mem, cst, U, zm, g, i, s, sg);
                        Vn[s] = v;
                        c = fmax(c, fabs(__dsub_rn(v, V[s])));
                        continue;
                    }
                    double acc = 0.0, bv = 0.0, qc = 0.0;
                    int ba = 0;
                    for (int k = 0; k < A; k++) {
                        const double qk = srn_q<MAXN>(a, s_mem, cst, U, zm, g, i, s, k);
                        if (mode == kMixed) {
                            acc = __dadd_rn(acc, __dmul_rn(srn_prob(a, s_mem, cst, g, i, s, k), qk));
                        } else {                         // the first maximum under strict >, and the incumbent's value
                            if (k == 0 || qk > bv) { bv = qk; ba = k; }
                            if (k == sg) qc = qk;
                        }
                    }
                    if (mode == kMixed) {
                        const double v = __ddiv_rn(acc, Si[s]);
                        Vn[s] = v;
                        c = fmax(c, fabs(__dsub_rn(v, V[s])));
                    } else if (bv > __dadd_rn(qc, margin)) {
                        sigma[s] = (uint16_t)ba;
                        c = 1.0;
                    }
                }
                c = sp_block_max(prod, cst, c, tid);
                if (mode == kImprove) {
                    if (!(c > 0.0)) { iters = n; break; } // no state changed: V* = V_n, sigma* = sigma_n
                    n++; m = 0; mode = kSigma;
                    continue;
                }
                double* tv = V; V = Vn; Vn = tv;
                m++;
                sweeps++;
                if (!(c <= a.eval_tol)) {
                    if (m >= a.max_sweeps) solved = false; // capped
                    continue;
                }
                if (mode == kMixed) {                    // V_pi: each thread wrote the states it copies
                    for (int s = tid; s < S; s += kSpBlock) Vpi[s] = V[s];
                    m = 0; mode = kSigma;
                } else if (n == THRL_EQ_MAX_ITERS) {
                    solved = false;
                } else {
                    mode = kImprove;
                }
            }
            __syncthreads();                             // Vpi, V and sigma of every thread

            if (!solved) {                               // a gamma outside [0, 1), or capped: NaN, br_policy = the modal action
                sr_flat_outputs(a, o, S, __builtin_nan(""), sweeps, modal, tid);
                __syncthreads();
                continue;
            }

            // ---- losses per state into the free V buffer, the weights w(s) over Z_-i (no longer read), then the
            // ordered sums: one lane each.  The weights depend on the game alone and are built again for every selected
            // agent: the working set has no array over the states to spare for them (Z_-i is the next agent's again),
            // and they are off the sweep path -- T reads of band per node against thousands of sweeps
            double* loss = Vn;
            double* wgt = Zm;
            const double* __restrict__ pig = a.pi ? a.pi + g * T : nullptr;
            for (int s = tid; s < S; s += kSpBlock) {
                sr_store_state(a, o, S, s, V, Vpi, sigma, loss);
                if (!pig) continue;
                if (s < D) {                             // w(d) = q M(d)
                    double M = 0.0;
                    const int e = first[s + 1];
                    for (int x = first[s]; x < e; x++) M = __dadd_rn(M, pig[perm[x]]);
                    wgt[s] = __dmul_rn(q, M);
                } else {                                 // w(D + j) = p nu(j), nu(j) = sum_t pi(t) nn(t, j)
                    const int64_t j = s - D;
                    double nu = 0.0;
                    for (int t = 0; t < T; t++) {
                        const int64_t w = j - a.band_lo[t];
                        if (w >= 0 && w < W) nu = __dadd_rn(nu, __dmul_rn(pig[t], a.band[(int64_t)t * W + w]));
                    }
                    wgt[s] = __dmul_rn(p, nu);
                }
            }
            __syncthreads();
            if (tid == 0) {
                double lmax = -__builtin_huge_val(), accd = 0.0, accn = 0.0;
                int ndd = 0, ndn = 0;
                sr_loss_range(loss, sigma, modal, 0, D, lmax, accd, ndd);
                sr_loss_range(loss, sigma, modal, D, S, lmax, accn, ndn);
                a.iters[o] = iters; a.sweeps[o] = sweeps;
                sr_summary(a, o, lmax, ndd, accd, ndn, accn);
            } else if (pig) {
                sr_weighted_sums(a, o, S, wgt, loss, V, Vpi, Si, sigma, tid,
                                 [&](int s, int k) THRL_SOLVE_INLINE { return srn_prob(a, s_mem, cst, g, i, s, k); });
            }
            __syncthreads();                             // loss / V / sigma reads before the next agent's writes
        }
    }
}

#ifndef THRL_SP_HOST_BUILD
template <int MAXN>
__global__ void __launch_bounds__(kSpBlock) k_srn_response(const SrnArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    srn_block<MAXN>(a, s_mem, (int)threadIdx.x, (int)blockIdx.x, (int)gridDim.x);
}
#endif

}  // namespace

#ifndef THRL_SP_HOST_BUILD
int launch_sampled_response_noise(const SrnArgs& a, int grid, hipStream_t s) {
    return sp_launch(k_srn_response<2>, k_srn_response<kSpMaxA>, a, a.sp, grid, s);
}
#endif

}  // namespace thrl
