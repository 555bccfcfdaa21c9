// thrl_attractors.hip -- attractor analysis of the greedy strategies (thrl_attractors, include/thrl.h): every limit
// cycle of a game's greedy map on the state set, its basin, its rewards, and the share of the reset distribution that
// ends in it.
//
// One wavefront (a one-wave block) per game, looping over games, lanes owning states s = lane, lane + 64, ...  The
// block keeps the per-config LUTs in LDS as k_equilibrium does: the state of every action tuple and, when it fits,
// every agent's reward per tuple.  Per game the wave gathers the policy entries of the state rows (2 bytes each, the
// only global reads besides the reset starts) and from then on works in LDS:
//   f = lev[0] lane-parallel, then L = ceil(log2 S) rounds of pointer doubling lev[k+1] = lev[k] o lev[k], every level
//   kept, with the running minimum over the orbit doubled alongside; 2^L >= S steps land every state on its cycle, so
//   the cycle states are the image of lev[L], rep(s) = the orbit minimum of where s lands, and mu(s) comes from
//   binary lifting over the stored levels (the last state of the path that is off every cycle).  Basin sizes and cycle
//   lengths are integer LDS adds keyed by rep, the kept attractors KEEP rounds of a wave-wide argmax on (basin, -rep).
// No state is walked step by step.  The only serial chains are the ones the definitions order: a cycle's reward sum
// (one lane per kept attractor, one lane per reset start) and the sums over the reset starts (one lane per output,
// reading the 64 starts of a chunk back from LDS).
#include "thrl_attractors.h"

#include "thrl_solve_dev.h"

namespace thrl {

namespace {

constexpr int kKeep = THRL_ATTR_KEEP;

struct AttrLds {
    const double* R;            // [N][T] rewards: LDS or global
    const uint16_t* pol;        // [N][S] greedy action of agent i in state s
    const uint16_t* tup;        // [S] tuple of the greedy actions in state s
    const uint16_t* f;          // [S] level 0
};

// (sum over the lam states of the cycle from r, in cycle order from 0.0) / lam, of agent i's reward and scaled action
__device__ __forceinline__ void cycle_mean(const AttrArgs& a, const AttrLds& v, int i, int r, int lam, double& cr,
                                           double& ca) {
    const AgentParams& p = a.ag[i];
    const double* __restrict__ R = v.R + (int64_t)i * a.T;
    const uint16_t* __restrict__ pol = v.pol + i * a.S;
    double sr = 0.0, sa = 0.0;
    int c = r;
    for (int j = 0; j < lam; j++) {
        sr = __dadd_rn(sr, R[v.tup[c]]);
        sa = __dadd_rn(sa, scale_action((int)pol[c], p));
        c = v.f[c];
    }
    cr = __ddiv_rn(sr, (double)lam);
    ca = __ddiv_rn(sa, (double)lam);
}

template <bool kLutLds>
__global__ void __launch_bounds__(64) k_attractors(const AttrArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    const int lane = threadIdx.x;
    const int S = a.S, N = a.N, TT = a.T, G = a.G, L = a.L, J = a.J;
    double* rlds = reinterpret_cast<double*>(s_mem + a.o_rew);
    double* cw = reinterpret_cast<double*>(s_mem + a.o_cw);           // [64] weight of the chunk's starts
    double* cprod = reinterpret_cast<double*>(s_mem + a.o_cprod);     // [N][64] w_j * cycle_reward_i
    int32_t* basin = reinterpret_cast<int32_t*>(s_mem + a.o_basin);
    int32_t* lamc = reinterpret_cast<int32_t*>(s_mem + a.o_lamc);
    int32_t* x0row = reinterpret_cast<int32_t*>(s_mem + a.o_x0row);
    int32_t* sel = reinterpret_cast<int32_t*>(s_mem + a.o_sel);       // [KEEP] rep of slot k, -1 = none
    int32_t* cslot = reinterpret_cast<int32_t*>(s_mem + a.o_cslot);   // [64] slot of the chunk's starts
    uint16_t* sid = reinterpret_cast<uint16_t*>(s_mem + a.o_sid);
    uint16_t* pol = reinterpret_cast<uint16_t*>(s_mem + a.o_pol);     // [N][S], then x_0's N actions
    uint16_t* lev = reinterpret_cast<uint16_t*>(s_mem + a.o_lev);     // [L + 1][S]: lev[k] = f^(2^k)
    uint16_t* ma = reinterpret_cast<uint16_t*>(s_mem + a.o_ma);
    uint16_t* mb = reinterpret_cast<uint16_t*>(s_mem + a.o_mb);
    uint16_t* rep = reinterpret_cast<uint16_t*>(s_mem + a.o_rep);
    uint16_t* mu = reinterpret_cast<uint16_t*>(s_mem + a.o_mu);
    uint16_t* on = reinterpret_cast<uint16_t*>(s_mem + a.o_on);       // 1: the state lies on a cycle
    uint16_t* tup = reinterpret_cast<uint16_t*>(s_mem + a.o_tup);
    int16_t* slotof = reinterpret_cast<int16_t*>(s_mem + a.o_slot);   // slot of the attractor with this rep, -1 = not kept

    for (int t = lane; t < TT; t += 64) sid[t] = a.sid[t];
    if constexpr (kLutLds)
        for (int j = lane; j < N * TT; j += 64) rlds[j] = a.rew[j];
    __syncthreads();
    AttrLds v;
    v.R = kLutLds ? rlds : a.rew;
    v.pol = pol;
    v.tup = tup;
    v.f = lev;

    for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
        const uint16_t* __restrict__ pg = a.policy + g * a.P;
        const double st = a.state0[g];

        // ---- the greedy action of every (agent, state) row and of x_0's rows (the policy word), the greedy map on
        // states, and x_0's place in it
        int t0;
        const int s0 = stage_game(a, st, pol, x0row, lane, [&](int i, int row) THRL_SOLVE_INLINE {
            return row_action(a, pg, i, row);
        }, [&](int s, int t) THRL_SOLVE_INLINE {
            tup[s] = (uint16_t)t;
            lev[s] = sid[t];
            ma[s] = (uint16_t)s;
            on[s] = 0;
            basin[s] = 0;
            lamc[s] = 0;
            slotof[s] = -1;
        }, t0);
        const int s1 = sid[t0];                          // x_1, a member whatever x_0 is
        __syncthreads();

        // ---- pointer doubling: lev[k + 1] = lev[k] o lev[k], and the minimum over the first 2^(k+1) orbit states
        uint16_t* mo = ma;
        uint16_t* mn = mb;
        for (int k = 0; k < L; k++) {
            double_min_round<64>(lev + k * S, lev + (k + 1) * S, mo, mn, S, lane);
            uint16_t* tm = mo; mo = mn; mn = tm;
        }
        const uint16_t* land = lev + L * S;             // f^(2^L), 2^L >= S: on a cycle from every state
        for (int s = lane; s < S; s += 64) on[land[s]] = 1;
        __syncthreads();

        // ---- rep and mu of every state; basin sizes and cycle lengths keyed by rep
        int mumax = 0, ncyc = 0, nattr = 0;
        for (int s = lane; s < S; s += 64) {
            const int r = mo[land[s]];
            int m = 0;
            if (!on[s]) {                                // the last state of the path that is off every cycle
                int cur = s;
                for (int k = L - 1; k >= 0; k--) {
                    const int nx = lev[k * S + cur];
                    if (!on[nx]) { cur = nx; m += 1 << k; }
                }
                m += 1;
            } else {
                atomicAdd(&lamc[r], 1);
                ncyc++;
            }
            atomicAdd(&basin[r], 1);
            rep[s] = (uint16_t)r;
            mu[s] = (uint16_t)m;
            nattr += r == s ? 1 : 0;
            mumax = max(mumax, m);
            if (a.state_rep) a.state_rep[g * S + s] = (uint16_t)r;
            if (a.state_mu) a.state_mu[g * S + s] = (uint16_t)m;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            mumax = max(mumax, __shfl_xor(mumax, m));
            ncyc += __shfl_xor(ncyc, m);
            nattr += __shfl_xor(nattr, m);
        }
        __syncthreads();

        // ---- the kept attractors: the largest (basin, -rep) below the one taken before, KEEP times
        uint32_t prev = 0xffffffffu;
        for (int k = 0; k < kKeep; k++) {
            const uint32_t best = keep_scan<64>(basin, rep, S, prev, lane);
            if (lane == 0) keep_take(best, k, sel, slotof);
            prev = best;                                 // 0 after the last attractor: nothing lies below it
        }
        __syncthreads();

        if (lane < kKeep) {
            const int r = sel[lane];
            const int lm = r >= 0 ? lamc[r] : 0;
            const int64_t o = (int64_t)lane * G + g;
            a.rep[o] = r;
            a.lam[o] = lm;
            a.basin[o] = r >= 0 ? basin[r] : 0;
            for (int i = 0; i < N; i++) {
                double cr = 0.0, ca = 0.0;
                if (r >= 0) cycle_mean(a, v, i, r, lm, cr, ca);
                const int64_t oi = ((int64_t)lane * N + i) * G + g;
                a.cycle_reward[oi] = cr;
                a.cycle_action[oi] = ca;
            }
        }
        if (lane == 0) {
            const int r = rep[s1];
            a.n_attr[g] = nattr;
            a.mu_max[g] = mumax;
            a.n_cycle_states[g] = ncyc;
            a.rep_x0[g] = r;
            a.mu_x0[g] = (s0 >= 0 && on[s0]) ? 0 : 1 + (int)mu[s1];
            a.slot_x0[g] = slotof[r];
        }

        // ---- the reset distribution: chunks of 64 starts, one lane per start, then one lane per ordered sum
        if (J > 0) {
            double acc = 0.0;
            for (int j0 = 0; j0 < J; j0 += 64) {
                const int j = j0 + lane;
                if (j < J) {
                    const int r = rep[sid[cell_tuple(a, pg, a.start_rows, J, j)]];
                    const double w = a.start_w[j];
                    const int lm = lamc[r];
                    cslot[lane] = slotof[r];
                    cw[lane] = w;
                    for (int i = 0; i < N; i++) {
                        double cr, ca;
                        cycle_mean(a, v, i, r, lm, cr, ca);
                        cprod[i * 64 + lane] = __dmul_rn(w, cr);
                    }
                }
                __syncthreads();
                acc = start_read_back<64>(cslot, cw, cprod, kKeep, N, min(64, J - j0), acc, lane);
                __syncthreads();
            }
            start_store(a.reset_mass, a.reset_mass_other, a.reset_reward, g, G, kKeep, N, lane, acc);
        }
        __syncthreads();                                 // this game's LDS reads before the next game's writes
    }
}

}  // namespace

int launch_attractors(const AttrArgs& a, int grid, hipStream_t s) {
    if (a.lut_lds)
        hipLaunchKernelGGL((k_attractors<true>), dim3(grid), dim3(64), (size_t)a.lds_bytes, s, a);
    else
        hipLaunchKernelGGL((k_attractors<false>), dim3(grid), dim3(64), (size_t)a.lds_bytes, s, a);
    return (int)hipGetLastError();
}

}  // namespace thrl
