// thrl_equilibrium.hip -- equilibrium check of the greedy strategies (thrl_equilibrium, include/thrl.h): for every
// game and agent, the exact best response to the rivals' greedy strategies by policy iteration on the state graph,
// and the value the agent's own greedy strategy gives up on the greedy path and anywhere.
//
// One wavefront (a one-wave block) per game, looping over games.  The block keeps the per-config LUTs in LDS: the state
// of every action tuple and, when it fits, every agent's reward per tuple (otherwise that one is read from global
// memory, where it stays cached).  Per game the wave stages the greedy action of every (agent, state) row -- the
// only reads of the tables, lane e taking entry e so a wave sweeps the window of rows front to back -- and from
// then on works in LDS with lanes owning states s = lane, lane + 64, ...  The policy evaluation by doubling keeps
// V and n in registers and gathers with ds_bpermute when S <= 64, and ping-pongs two LDS copies otherwise; both
// do the same operations on the same values.  Everything a lane does alone (the cycle walk, the ordered sums) is
// done by all lanes on the same LDS words, so no result has to be broadcast.
#include "thrl_equilibrium.h"

#include "thrl_solve_dev.h"

namespace thrl {

namespace {

// argmax_row (first maximum under strict >) with eight loads in flight; reads row[0 .. n) only
template <typename T>
__device__ __forceinline__ int argmax_row8(const T* __restrict__ row, int n) {
    int b = 0;
    T bv = row[0];
    for (int k0 = 0; k0 < n; k0 += 8) {
        T v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = row[min(k0 + j, n - 1)];
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (k0 + j < n && v[j] > bv) { bv = v[j]; b = k0 + j; }
    }
    return b;
}

template <typename T, bool kSmall, bool kLutLds>
__global__ void __launch_bounds__(64) k_equilibrium(const EqArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    const int lane = threadIdx.x;
    const int S = a.S, N = a.N, TT = a.T, G = a.G;
    double* Va = reinterpret_cast<double*>(s_mem + a.o_va);
    double* Vb = reinterpret_cast<double*>(s_mem + a.o_vb);
    double* Vpi = reinterpret_cast<double*>(s_mem + a.o_vpi);
    double* rlds = reinterpret_cast<double*>(s_mem + a.o_rew);
    int32_t* base = reinterpret_cast<int32_t*>(s_mem + a.o_base);
    int16_t* first = reinterpret_cast<int16_t*>(s_mem + a.o_first);   // step at which the walk met the state
    int32_t* x0row = reinterpret_cast<int32_t*>(s_mem + a.o_x0row);
    uint16_t* sid = reinterpret_cast<uint16_t*>(s_mem + a.o_sid);
    uint16_t* pol = reinterpret_cast<uint16_t*>(s_mem + a.o_pol);       // [N][S], then x_0's N actions
    uint16_t* sigma = reinterpret_cast<uint16_t*>(s_mem + a.o_sigma);
    uint16_t* jn = reinterpret_cast<uint16_t*>(s_mem + a.o_jn);
    uint16_t* na = reinterpret_cast<uint16_t*>(s_mem + a.o_na);
    uint16_t* nb = reinterpret_cast<uint16_t*>(s_mem + a.o_nb);
    const T* __restrict__ qbase = reinterpret_cast<const T*>(a.q);

    for (int t = lane; t < TT; t += 64) sid[t] = a.sid[t];
    if constexpr (kLutLds)
        for (int j = lane; j < N * TT; j += 64) rlds[j] = a.rew[j];
    __syncthreads();

    for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
        const T* __restrict__ qg = qbase + g * a.stride;
        const double st = a.state0[g];

        // ---- the greedy action of every (agent, state) row and of x_0's rows (the argmax of the table row), the joint
        // greedy map on states, x_0's place in it, and the cycle
        int t0;
        const int s0 = stage_game(a, st, pol, x0row, lane, [&](int i, int row) THRL_SOLVE_INLINE {
            const AgentParams& p = a.ag[i];
            return argmax_row8(qg + p.table_off + (int64_t)row * p.n_actions, p.n_actions);
        }, [&](int s, int t) THRL_SOLVE_INLINE {
            jn[s] = sid[t];
            first[s] = -1;
        }, t0);
        __syncthreads();
        int cur = s0 >= 0 ? s0 : (int)sid[t0];
        int tm = s0 >= 0 ? 0 : 1;
        int mu = 0, lam = 1;
        for (int guard = 0; guard <= S; guard++) {       // every lane walks the same words (first_visit_walk's lines, inline:
            const int f = first[cur];                    // through the function the launch is 1 % slower)
            if (f >= 0) { mu = f; lam = tm - f; break; }
            first[cur] = (int16_t)tm;
            cur = jn[cur];
            tm++;
        }
        const int c0 = cur;                              // x_mu
        if (lane == 0) { a.mu[g] = mu; a.lam[g] = lam; }

        for (int i = 0; i < N; i++) {
            if (!((a.agents >> i) & 1)) continue;
            const int64_t o = (int64_t)i * G + g;
            const double gam = a.sweep_gamma ? a.sweep_gamma[o] : a.ag[i].gamma;
            if (!(gam >= 0.0 && gam < 1.0)) {
                if (lane == 0) store_agent_unsolved(a, o);
                continue;
            }
            const int D = doubling_rounds(gam);
            const int nact = a.ag[i].n_actions, ts = a.tstride[i];
            const double* __restrict__ R = (kLutLds ? rlds : a.rew) + (int64_t)i * TT;

            for (int s = lane; s < S; s += 64) {
                int t = 0;
                for (int j = 0; j < N; j++)
                    if (j != i) t += (int)pol[j * S + s] * a.tstride[j];
                base[s] = t;
                sigma[s] = pol[i * S + s];
            }

            const auto succ = [&](int t) THRL_SOLVE_INLINE { return (int)sid[t]; };    // the state a tuple leads to
            double* V = Va;                              // where the evaluation leaves V
            int iters = -1;
            for (int k = 0;; k++) {
                // ---- V = evaluation of sigma
                if constexpr (kSmall) {
                    double v = 0.0;
                    int n = lane;
                    if (lane < S) {
                        const int t = base[lane] + (int)sigma[lane] * ts;
                        v = R[t];
                        n = sid[t];
                    }
                    double w = gam;
                    for (int d = 0; d < D; d++) {
                        const double vm = __shfl(v, n);
                        const int nn = __shfl(n, n);
                        v = __dadd_rn(v, __dmul_rn(w, vm));
                        n = nn;
                        w = __dmul_rn(w, w);
                    }
                    if (lane < S) Va[lane] = v;
                    __syncthreads();
                } else {
                    V = eval_doubling<64>(Va, Vb, na, nb, base, sigma, ts, R, S, D, gam, lane, succ);
                }
                if (k == 0)
                    for (int s = lane; s < S; s += 64) Vpi[s] = V[s];
                if (k == THRL_EQ_MAX_ITERS) break;

                // ---- improvement: keep the incumbent unless some action is strictly better
                // (improve_strict's lines, inline: through the function this kernel's launch is 4 % slower)
                bool changed = false;
                for (int s = lane; s < S; s += 64) {
                    const int b = base[s];
                    const int tc = b + (int)sigma[s] * ts;
                    const double qc = __dadd_rn(R[tc], __dmul_rn(gam, V[sid[tc]]));
                    double bv = __dadd_rn(R[b], __dmul_rn(gam, V[sid[b]]));
                    int ba = 0;
                    for (int act = 1; act < nact; act++) {
                        const int t = b + act * ts;
                        const double qv = __dadd_rn(R[t], __dmul_rn(gam, V[sid[t]]));
                        if (qv > bv) { bv = qv; ba = act; }
                    }
                    if (bv > qc) { sigma[s] = (uint16_t)ba; changed = true; }
                }
                const bool any = __ballot(changed) != 0;
                __syncthreads();                         // every read of V before the next evaluation overwrites it
                if (!any) { iters = k; break; }
            }
            __syncthreads();                             // Vpi and sigma of every lane

            // ---- losses: per state into the free V buffer, then the ordered sums
            double* loss = (V == Va) ? Vb : Va;
            int nd = 0;
            double lmax = -__builtin_huge_val();
            for (int s = lane; s < S; s += 64) {
                const double vs = V[s], vp = Vpi[s];
                const double l = rel_loss(vs, vp);
                loss[s] = l;
                if (l > lmax) lmax = l;
                nd += sigma[s] != pol[i * S + s] ? 1 : 0;
                store_state(a, o * S + s, sigma[s], vs, vp);
            }
            wave_max_sum(lmax, nd);
            __syncthreads();
            double sum_all = 0.0;
            for (int s = 0; s < S; s++) sum_all = __dadd_rn(sum_all, loss[s]);
            const OnCycle on = on_cycle_sums(loss, Vpi, jn, c0, lam, [&](int c) THRL_SOLVE_INLINE {
                return sigma[c] != pol[i * S + c] ? 1 : 0;
            });
            if (lane == 0) {
                a.iters[o] = iters;
                a.n_diff_all[o] = nd;
                a.n_diff_on[o] = on.nd;
                a.loss_all[o] = lmax;
                a.loss_on[o] = on.lon;
                a.loss_all_mean[o] = __ddiv_rn(sum_all, (double)S);
                a.loss_on_mean[o] = __ddiv_rn(on.sum, (double)lam);
                a.v_on[o] = __ddiv_rn(on.von, (double)lam);
            }
            __syncthreads();                             // loss / V / sigma reads before the next agent's writes
        }
        __syncthreads();                                 // this game's LDS reads before the next game's writes
    }
}

template <typename T, bool kSmall>
void launch_l(const EqArgs& a, int grid, hipStream_t s) {
    if (a.lut_lds)
        hipLaunchKernelGGL((k_equilibrium<T, kSmall, true>), dim3(grid), dim3(64), (size_t)a.lds_bytes, s, a);
    else
        hipLaunchKernelGGL((k_equilibrium<T, kSmall, false>), dim3(grid), dim3(64), (size_t)a.lds_bytes, s, a);
}

template <typename T>
void launch_t(const EqArgs& a, int grid, hipStream_t s) {
    if (a.small) launch_l<T, true>(a, grid, s);
    else launch_l<T, false>(a, grid, s);
}

}  // namespace

int launch_equilibrium(const EqArgs& a, int q_dtype, int grid, hipStream_t s) {
    if (q_dtype == 1) launch_t<double>(a, grid, s);
    else launch_t<float>(a, grid, s);
    return (int)hipGetLastError();
}

}  // namespace thrl
