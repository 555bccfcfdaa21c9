// thrl_tuple_attractors.hip -- attractor analysis of strategies in tuple form (thrl_tuple_attractors, include/thrl.h):
// thrl_attractors for any mix of QTable, Reinforce and ActorCritic agents, with the T action tuples as the state set.
// Every limit cycle of a game's greedy map F on tuple indices, its basin, its rewards, and the share of a caller's
// start weights that ends in it.  No encode, no network and no env arithmetic: rewards and scaled actions are looked
// up in the caller's per-config tables, which stay in global memory (L2); only F lives in LDS.
//
// k_ta_attractors: one 256-thread block per game, looping over games; threads own the tuples s = tid, tid + 256, ..
// The state set is up to four times thrl_attractors' 1024 states and every doubling round depends on the whole
// previous round, so four waves share a game.  k_attractors keeps every doubling level to binary-lift mu; at T = 4096
// that store alone is 13 x 8 KB, so here two doubling passes share one pair of ping-pong buffers:
//   pass 1  p = F, m(s) = s; L = ceil(log2 T) rounds p' = p o p, m' = min(m, m o p).  2^L >= T steps land every tuple on
//           its cycle and cover the cycle, so the cycle tuples are the image of p and rep(s) = m(p(s)).
//   pass 2  the absorbed map h(s) = s on a cycle, else F(s), with the step count d(s) = 0 / 1; L rounds d' = d + d o h,
//           h' = h o h.  d counts the off-cycle tuples among the first 2^L of the path: mu.
// Basin sizes and cycle lengths are integer LDS adds keyed by rep, the kept attractors KEEP rounds of a block-wide argmax
// on (basin, -rep).  The only serial chains are the ones the definitions order: a cycle's reward sum (one lane per kept
// slot and agent; the means are cached for the start weights, and only a tuple whose attractor is not kept walks its
// cycle) and the sums over the start weights (one lane per output, reading the 256 terms of a chunk back from LDS).
// Nothing depends on the grid size or on which block takes which game.
#include "thrl_tuple_attractors.h"

#include "thrl_solve_dev.h"

namespace thrl {

namespace {

constexpr int kKeep = THRL_ATTR_KEEP;

// (sum over the lam tuples F(r), F^2(r), .., F^lam(r) = r, in that order from 0.0) / lam of the table row tab
__device__ __forceinline__ double tat_cycle_mean(const uint16_t* __restrict__ F, const double* __restrict__ tab, int r,
                                                 int lam) {
    double s = 0.0;
    int c = r;
    for (int j = 0; j < lam; j++) {
        c = F[c];
        s = __dadd_rn(s, tab[c]);
    }
    return __ddiv_rn(s, (double)lam);
}

__global__ void __launch_bounds__(kTatBlock) k_ta_attractors(const TatArgs a) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    constexpr int B = kTatBlock;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.T, N = a.N, G = a.G, L = a.L;
    double* cw = reinterpret_cast<double*>(s_mem + a.o_cw);             // [B] weight of the chunk's tuples
    double* cprod = reinterpret_cast<double*>(s_mem + a.o_cprod);       // [N][B] w_t * cycle_reward_i
    double* cmean = reinterpret_cast<double*>(s_mem + a.o_cmean);       // [KEEP][N] cycle_reward of the kept slots
    int32_t* basin = reinterpret_cast<int32_t*>(s_mem + a.o_basin);
    int32_t* lamc = reinterpret_cast<int32_t*>(s_mem + a.o_lamc);
    int32_t* sel = reinterpret_cast<int32_t*>(s_mem + a.o_sel);         // [KEEP] rep of slot k, -1 = none
    int32_t* red = reinterpret_cast<int32_t*>(s_mem + a.o_red);         // [8] argmax keys (two rounds), [3][4] per-wave counts
    uint16_t* F = reinterpret_cast<uint16_t*>(s_mem + a.o_f);
    uint16_t* pa = reinterpret_cast<uint16_t*>(s_mem + a.o_pa);
    uint16_t* pb = reinterpret_cast<uint16_t*>(s_mem + a.o_pb);
    uint16_t* ma = reinterpret_cast<uint16_t*>(s_mem + a.o_ma);
    uint16_t* mb = reinterpret_cast<uint16_t*>(s_mem + a.o_mb);
    uint16_t* rep = reinterpret_cast<uint16_t*>(s_mem + a.o_rep);
    uint16_t* on = reinterpret_cast<uint16_t*>(s_mem + a.o_on);         // 1: the tuple lies on a cycle
    int16_t* slotof = reinterpret_cast<int16_t*>(s_mem + a.o_slot);     // slot of the attractor with this rep, -1 = not kept
    int16_t* cslot = reinterpret_cast<int16_t*>(s_mem + a.o_cslot);     // [B] slot of the chunk's tuples

    for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
        const uint16_t* __restrict__ pg = a.policy + g * N * T;

        // ---- the greedy map
        for (int s = tid; s < T; s += B) {
            const int t = tuple_map(a, pg, T, s, -1);
            F[s] = (uint16_t)t;
            pa[s] = (uint16_t)t;
            ma[s] = (uint16_t)s;
            on[s] = 0;
            basin[s] = 0;
            lamc[s] = 0;
            slotof[s] = -1;
        }
        __syncthreads();

        // ---- pass 1: p = F^(2^k), m = the minimum over the first 2^k tuples of the orbit
        uint16_t* po = pa;
        uint16_t* pn = pb;
        uint16_t* mo = ma;
        uint16_t* mn = mb;
        for (int k = 0; k < L; k++) {
            double_min_round<B>(po, pn, mo, mn, T, tid);
            uint16_t* tp = po; po = pn; pn = tp;
            uint16_t* tm = mo; mo = mn; mn = tm;
        }
        for (int s = tid; s < T; s += B) on[po[s]] = 1;  // p = F^(2^L), 2^L >= T: on a cycle from every tuple
        __syncthreads();

        // ---- rep of every tuple, basin sizes and cycle lengths keyed by rep; the absorbed map into the free buffers
        int mumax = 0, ncyc = 0, nattr = 0;
        for (int s = tid; s < T; s += B) {
            const int r = mo[po[s]];
            const int o = on[s];
            rep[s] = (uint16_t)r;
            atomicAdd(&basin[r], 1);
            if (o) {
                atomicAdd(&lamc[r], 1);
                ncyc++;
            }
            nattr += r == s ? 1 : 0;
            pn[s] = o ? (uint16_t)s : F[s];
            mn[s] = o ? 0 : 1;
        }
        __syncthreads();

        // ---- pass 2: h = h0^(2^k), d = the off-cycle tuples among the first 2^k of the path
        uint16_t* ho = pn;
        uint16_t* hn = po;
        uint16_t* dold = mn;
        uint16_t* dnew = mo;
        for (int k = 0; k < L; k++) {
            for (int s = tid; s < T; s += B) {
                const int m = ho[s];
                hn[s] = ho[m];
                dnew[s] = (uint16_t)((int)dold[s] + (int)dold[m]);
            }
            __syncthreads();
            uint16_t* th = ho; ho = hn; hn = th;
            uint16_t* td = dold; dold = dnew; dnew = td;
        }
        const uint16_t* mu = dold;
        for (int s = tid; s < T; s += B) {
            const int m = mu[s];
            mumax = max(mumax, m);
            if (a.tuple_rep) a.tuple_rep[g * T + s] = rep[s];
            if (a.tuple_mu) a.tuple_mu[g * T + s] = (uint16_t)m;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            mumax = max(mumax, __shfl_xor(mumax, m));
            ncyc += __shfl_xor(ncyc, m);
            nattr += __shfl_xor(nattr, m);
        }
        if (lane == 0) {
            red[8 + wave] = mumax;
            red[12 + wave] = ncyc;
            red[16 + wave] = nattr;
        }

        // ---- the kept attractors: the largest (basin, -rep) below the one taken before, KEEP times
        uint32_t prev = 0xffffffffu;
        for (int k = 0; k < kKeep; k++) {
            uint32_t best = keep_scan<B>(basin, rep, T, prev, tid);
            int32_t* rk = red + (k & 1) * 4;            // two rounds apart: the barrier between ends every read
            if (lane == 0) rk[wave] = (int32_t)best;
            __syncthreads();
            best = max(max((uint32_t)rk[0], (uint32_t)rk[1]), max((uint32_t)rk[2], (uint32_t)rk[3]));
            if (tid == 0) keep_take(best, k, sel, slotof);
            prev = best;                                 // 0 after the last attractor: nothing lies below it
        }
        __syncthreads();

        // ---- the kept slots: one lane per (slot, agent) walks the cycle; the reward means are kept for the start weights
        if (tid < kKeep * N) {
            const int k = tid / N, i = tid - k * N;
            const int r = sel[k];
            const int lm = r >= 0 ? lamc[r] : 0;
            double cr = 0.0, ca = 0.0;
            if (r >= 0) {
                cr = tat_cycle_mean(F, a.reward + (int64_t)i * T, r, lm);
                ca = tat_cycle_mean(F, a.scaled + (int64_t)i * T, r, lm);
            }
            const int64_t oi = ((int64_t)k * N + i) * G + g;
            a.cycle_reward[oi] = cr;
            a.cycle_action[oi] = ca;
            cmean[k * N + i] = cr;
            if (i == 0) {
                const int64_t o = (int64_t)k * G + g;
                a.rep[o] = r;
                a.lam[o] = lm;
                a.basin[o] = r >= 0 ? basin[r] : 0;
            }
        }
        if (tid == 0) {
            const int t0 = a.start[g];
            const bool ok = t0 >= 0 && t0 < T;
            const int r = ok ? (int)rep[t0] : -1;
            a.n_attr[g] = red[16] + red[17] + red[18] + red[19];
            a.mu_max[g] = max(max(red[8], red[9]), max(red[10], red[11]));
            a.n_cycle_states[g] = red[12] + red[13] + red[14] + red[15];
            a.rep_x0[g] = r;
            a.mu_x0[g] = ok ? (int)mu[t0] : -1;
            a.slot_x0[g] = ok ? (int)slotof[r] : -1;
        }

        // ---- the start weights: chunks of 256 tuples, one thread per tuple, then one lane per ordered sum
        if (a.start_w) {
            __syncthreads();                             // cmean
            double acc = 0.0;
            for (int j0 = 0; j0 < T; j0 += B) {
                const int t = j0 + tid;
                if (t < T) {
                    const int r = rep[t];
                    const int sl = slotof[r];
                    const double w = a.start_w[t];
                    cslot[tid] = (int16_t)sl;
                    cw[tid] = w;
                    const int lm = sl < 0 ? lamc[r] : 0;
                    for (int i = 0; i < N; i++) {
                        const double cr = sl >= 0 ? cmean[sl * N + i] : tat_cycle_mean(F, a.reward + (int64_t)i * T, r, lm);
                        cprod[i * B + tid] = __dmul_rn(w, cr);
                    }
                }
                __syncthreads();
                acc = start_read_back<B>(cslot, cw, cprod, kKeep, N, min(B, T - j0), acc, tid);
                __syncthreads();
            }
            start_store(a.start_mass, a.start_mass_other, a.start_reward, g, G, kKeep, N, tid, acc);
        }
        __syncthreads();                                 // this game's LDS reads before the next game's writes
    }
}

}  // namespace

int launch_tuple_attractors(const TatArgs& a, int grid, hipStream_t s) {
    if (a.lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_ta_attractors),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, a.lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k_ta_attractors, dim3(grid), dim3(kTatBlock), (size_t)a.lds_bytes, s, a);
    return (int)hipGetLastError();
}

}  // namespace thrl
