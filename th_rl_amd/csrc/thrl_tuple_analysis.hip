// thrl_tuple_analysis.hip -- the deviation test and the equilibrium check for strategies in tuple form
// (thrl_tuple_deviation, thrl_tuple_equilibrium, include/thrl.h): thrl_deviation and thrl_equilibrium for any mix of
// QTable, Reinforce and ActorCritic agents, on the uint16 tables thrl_tuple_policy writes.  No encode, no network and
// no env arithmetic: rewards and scaled actions are looked up in the caller's per-config tables.  Two kernels.
//
// k_ta_deviation: one lane per game, k_tp_walk's shape.  The walk (the cycle search, the deviation and baseline paths
//   in lockstep, the return) runs on a single integer; the 2-byte policy entries it visits are gathered from global
//   memory and the reward / scaled tables sit in LDS when they fit kTaDevLdsBudget.  The map on tuple indices, the
//   search, the means over the cycle, the refused game's zeros, the store of the row slice and the staging of the
//   tables are thrl_walk_dev.h's; the lockstep loop is this file's.
// k_ta_equilibrium: one 256-thread block per game, looping over games; lanes own the states s = tid, tid + 256, ..
//   (at most 16 each).  The state set is the T tuples, up to four times thrl_equilibrium's 1024 states, and every
//   doubling pass of an evaluation depends on the whole previous pass, so four waves share a game.  LDS holds, per
//   tuple, the two V buffers and the two jump tables of the evaluation, sigma, the joint map, the other agents' base
//   tuple and the solved agent's reward row: 36 bytes, 144 KB at T = 4096.  The strategies themselves are read from
//   tuple_policy with coalesced loads (a handful of sweeps per agent), and V_pi stays in the owning lane's registers
//   until the losses are formed; it then replaces V* in LDS for the sums along the cycle.  What has to be done in a
//   stated order is done by one wave alone: wave 0 walks the path and adds the losses in state order, wave 1 adds
//   along the cycle.  Nothing depends on the grid size or on which block takes which game.
#include "thrl_tuple_analysis.h"

#include "thrl_solve_dev.h"
#include "thrl_walk_dev.h"

namespace thrl {

namespace {

// ------------------------------------------------------------------------------------------------ deviation
template <bool kLds, int MAXN>
__global__ void __launch_bounds__(kTaDevTile) k_ta_deviation(const TaDevArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    const int tid = threadIdx.x;
    const int G = a.G, N = a.N, T = a.T;
    const double* rew = a.reward;
    const double* sca = a.scaled;
    if constexpr (kLds) stage_tables(s_mem, N * T, tid, kTaDevTile, rew, sca);
    const int64_t g = (int64_t)blockIdx.x * kTaDevTile + tid;
    if (g >= G) return;
    const int t0 = a.start[g];

    if (t0 < 0 || t0 >= T) {                            // the stated refusal: nothing of the game is read
        a.mu[g] = -1;
        a.lam[g] = 0;
        a.mu_post[g] = 0;
        a.lam_post[g] = 0;
        a.ret_step[g] = -1;
        a.act_dev[g] = -1;
        a.gain[g] = 0.0;
        store_refused(a, g, G);
        return;
    }

    TupleView<MAXN> v;              // this lane's game
#pragma unroll
    for (int i = 0; i < MAXN; i++)
        v.gp[i] = a.policy + (g * N + (i < N ? i : 0)) * T;
    // t <- the index of the tuple the game's agents play at t, and where the values of that tuple lie
    const auto next = [&](int& t) THRL_WALK_INLINE {
        t = tuple_next<MAXN>(a, v, t);
        return StepOut{rew + t, sca + t, T};
    };

    // pre-shock cycle
    int mu, lam, s;
    find_cycle(t0, N, a.H, next, mu, lam, s, true);
    double cr[MAXN], ca[MAXN];
    int x = s;
    cycle_means<MAXN>(N, lam, cr, ca, [&]() THRL_WALK_INLINE { return next(x); });

    // deviation path y and baseline path z, in lockstep
    const int d = a.d, L = a.L, K = a.K;
    const int nd = a.n_actions[d], tsd = a.tstride[d];
    const double* rd = rew + d * T;
    const double gam = a.sweep_gamma ? a.sweep_gamma[(int64_t)d * G + g] : a.gamma_d;
    int y = s, z = s, yL = s;
    double gain = 0.0, w = 1.0;
    int adev = 0;
    for (int t = 0; t < K; t++) {
        if (t < L) {
            int ub = 0;                                 // the others greedy at y
#pragma unroll
            for (int i = 0; i < MAXN; i++)
                if (i < N && i != d) ub += tuple_act<MAXN>(a, v, i, y) * a.tstride[i];
            int ad = a.dev_action;
            if (ad < 0) {                               // one-period best response: first maximum of d's reward
                double bv = 0.0;
                ad = 0;
                for (int k = 0; k < nd; k++) {
                    const double r = rd[ub + k * tsd];
                    if (k == 0 || r > bv) { bv = r; ad = k; }
                }
            }
            if (t == 0) adev = ad;
            y = ub + ad * tsd;
        } else {
            next(y);
        }
        store_step<MAXN>(a, t, g, G, StepOut{rew + y, sca + y, T});
        next(z);
        gain = __dadd_rn(gain, __dmul_rn(w, __dsub_rn(rd[y], rd[z])));
        w = __dmul_rn(w, gam);
        if (t + 1 == L) yL = y;
    }

    // return to the pre-shock cycle
    int mp, lp, sp = 0;
    const bool fp = find_cycle(yL, N, a.H, next, mp, lp, sp, false);
    int ret = -1;
    if (lam > 0 && fp) {
        for (int j = 0; j < lp; j++) {
            if (sp == s) { ret = L + mp; break; }
            next(sp);
        }
    }

    a.mu[g] = mu;
    a.lam[g] = lam;
    a.mu_post[g] = mp;
    a.lam_post[g] = lp;
    a.ret_step[g] = ret;
    a.act_dev[g] = adev;
    a.gain[g] = gain;
    store_means<MAXN>(a, g, G, cr, ca);
}

template <bool kLds>
void launch_dev_n(const TaDevArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)(((int64_t)a.G + kTaDevTile - 1) / kTaDevTile)), block(kTaDevTile);
    const size_t lds = (size_t)a.lds_bytes;
    if (a.N <= 2) hipLaunchKernelGGL((k_ta_deviation<kLds, 2>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((k_ta_deviation<kLds, THRL_MAXA>), grid, block, lds, s, a);
}

// ------------------------------------------------------------------------------------------------ equilibrium
__global__ void __launch_bounds__(kTaEqBlock) k_ta_equilibrium(const TaEqArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    constexpr int B = kTaEqBlock;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.T, N = a.N, G = a.G;
    double* Va = reinterpret_cast<double*>(s_mem + a.o_va);
    double* Vb = reinterpret_cast<double*>(s_mem + a.o_vb);
    double* R = reinterpret_cast<double*>(s_mem + a.o_rew);             // the solved agent's reward per tuple
    uint16_t* na = reinterpret_cast<uint16_t*>(s_mem + a.o_na);
    uint16_t* nb = reinterpret_cast<uint16_t*>(s_mem + a.o_nb);
    uint16_t* sigma = reinterpret_cast<uint16_t*>(s_mem + a.o_sigma);
    uint16_t* jn = reinterpret_cast<uint16_t*>(s_mem + a.o_jn);         // F
    int16_t* mark = reinterpret_cast<int16_t*>(s_mem + a.o_mark);       // walk: step of the first visit; then sigma* != pi_i
    uint16_t* base = reinterpret_cast<uint16_t*>(s_mem + a.o_base);     // the tuple of the others' actions, 0 in place i
    double* red_d = reinterpret_cast<double*>(s_mem + a.o_misc);        // [4] per-wave maxima
    int32_t* red_i = reinterpret_cast<int32_t*>(s_mem + a.o_misc + 32); // [4] per-wave counts, then mu, lam, t_mu
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
        const uint16_t* __restrict__ pg = a.policy + g * N * T;

        // ---- the joint greedy map, and the path from the start tuple (wave 0 alone: its lanes walk the same words)
        for (int s = tid; s < T; s += B) {
            jn[s] = (uint16_t)tuple_map(a, pg, T, s, -1);
            mark[s] = -1;
        }
        __syncthreads();
        if (wave == 0) {
            const int t0 = a.start[g];
            int mu = -1, lam = 0, cur = 0;
            if (t0 >= 0 && t0 < T) cur = first_visit_walk(mark, jn, T, t0, 0, mu, lam);
            if (lane == 0) {
                red_i[4] = mu; red_i[5] = lam; red_i[6] = cur;
                a.mu[g] = mu;
                a.lam[g] = lam;
            }
        }
        __syncthreads();
        const int lam = red_i[5], c0 = red_i[6];

        for (int i = 0; i < N; i++) {
            if (!((a.agents >> i) & 1)) continue;
            const int64_t o = (int64_t)i * G + g;
            const double gam = a.sweep_gamma ? a.sweep_gamma[o] : a.gamma[i];
            if (!(gam >= 0.0 && gam < 1.0)) {
                if (tid == 0) store_agent_unsolved(a, o);
                continue;
            }
            const int D = doubling_rounds(gam);
            const int nact = a.n_actions[i], ts = a.tstride[i];
            const uint16_t* __restrict__ pi = pg + i * T;
            const double* __restrict__ Rg = a.reward + (int64_t)i * T;

            for (int s = tid; s < T; s += B) {
                base[s] = (uint16_t)tuple_map(a, pg, T, s, i);
                sigma[s] = (uint16_t)min((int)pi[s], nact - 1);
                R[s] = Rg[s];
            }
            __syncthreads();

            const auto succ = [](int t) THRL_SOLVE_INLINE { return t; };    // a tuple is the state it leads to
            double vpi[kTaEqMaxPerLane];                 // V_pi of this lane's states
            double* V = Va;
            int iters = -1;
            for (int k = 0;; k++) {
                // ---- V = evaluation of sigma
                V = eval_doubling<B>(Va, Vb, na, nb, base, sigma, ts, R, T, D, gam, tid, succ);
                if (k == 0) {
#pragma unroll
                    for (int kk = 0; kk < kTaEqMaxPerLane; kk++) {
                        const int s = tid + kk * B;
                        vpi[kk] = s < T ? V[s] : 0.0;
                    }
                }
                if (k == THRL_EQ_MAX_ITERS) break;

                // ---- improvement: keep the incumbent unless some action is strictly better
                const int changed = improve_strict<B>(base, sigma, ts, nact, R, V, T, gam, tid, succ) ? 1 : 0;
                // the barrier also ends every read of V before the next evaluation overwrites it
                if (!__syncthreads_or(changed)) { iters = k; break; }
            }

            // ---- losses: per state into the free V buffer; then V_pi takes V*'s place for the sums along the cycle
            double* loss = (V == Va) ? Vb : Va;
            int nd = 0;
            double lmax = -__builtin_huge_val();
#pragma unroll
            for (int kk = 0; kk < kTaEqMaxPerLane; kk++) {
                const int s = tid + kk * B;
                if (s < T) {
                    const double vs = V[s], vp = vpi[kk];
                    const double l = rel_loss(vs, vp);
                    loss[s] = l;
                    if (l > lmax) lmax = l;
                    const int diff = (int)sigma[s] != min((int)pi[s], nact - 1) ? 1 : 0;
                    mark[s] = (int16_t)diff;
                    nd += diff;
                    store_state(a, o * T + s, sigma[s], vs, vp);
                }
            }
            wave_max_sum(lmax, nd);
            if (lane == 0) { red_d[wave] = lmax; red_i[wave] = nd; }
            __syncthreads();                             // every read of V* is done
#pragma unroll
            for (int kk = 0; kk < kTaEqMaxPerLane; kk++) {
                const int s = tid + kk * B;
                if (s < T) V[s] = vpi[kk];
            }
            __syncthreads();
            if (wave == 0) {                             // all states, in state order
                double sum_all = 0.0;
                for (int s = 0; s < T; s++) sum_all = __dadd_rn(sum_all, loss[s]);
                if (lane == 0) {
                    double lm = red_d[0];
                    int ndall = red_i[0];
                    for (int wv = 1; wv < B / 64; wv++) {
                        if (red_d[wv] > lm) lm = red_d[wv];
                        ndall += red_i[wv];
                    }
                    a.iters[o] = iters;
                    a.n_diff_all[o] = ndall;
                    a.loss_all[o] = lm;
                    a.loss_all_mean[o] = __ddiv_rn(sum_all, (double)T);
                }
            } else if (wave == 1) {                      // the cycle, in cycle order
                const OnCycle on = on_cycle_sums(loss, V, jn, c0, lam, [&](int c) THRL_SOLVE_INLINE { return (int)mark[c]; });
                if (lane == 0) {
                    a.n_diff_on[o] = on.nd;
                    a.loss_on[o] = lam > 0 ? on.lon : nan;
                    a.loss_on_mean[o] = lam > 0 ? __ddiv_rn(on.sum, (double)lam) : nan;
                    a.v_on[o] = lam > 0 ? __ddiv_rn(on.von, (double)lam) : nan;
                }
            }
            __syncthreads();                             // loss / V / mark reads before the next agent's writes
        }
        __syncthreads();                                 // this game's LDS reads before the next game's writes
    }
}

}  // namespace

int launch_ta_deviation(const TaDevArgs& a, hipStream_t s) {
    if (a.in_lds) launch_dev_n<true>(a, s);
    else launch_dev_n<false>(a, s);
    return (int)hipGetLastError();
}

int launch_ta_equilibrium(const TaEqArgs& a, int grid, hipStream_t s) {
    if (a.lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_ta_equilibrium),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, a.lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k_ta_equilibrium, dim3(grid), dim3(kTaEqBlock), (size_t)a.lds_bytes, s, a);
    return (int)hipGetLastError();
}

}  // namespace thrl
