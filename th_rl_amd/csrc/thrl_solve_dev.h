// thrl_solve_dev.h -- the pieces the six kernels that solve a game's whole state graph share word for word:
// k_equilibrium, k_ta_equilibrium (thrl_tuple_analysis.hip), k_equilibrium_noise, k_tuple_equilibrium_noise, k_attractors
// and k_ta_attractors (thrl_tuple_attractors.hip).  Threads own the states s = tid, tid + B, .., B = 64 in the one-wave
// kernels and 256 in the tuple kernels.  The kernels' bodies, their LDS layouts, k_equilibrium's register path, the two
// ways to mu, stage_x, every cross-wave reduction and the cycle means (k_attractors adds two tables in one walk from r,
// k_ta_attractors one table from F(r): the same adds in another order) stay in the kernels.  Device inline functions
// only, in namespace thrl's anonymous namespace, once per including file.  A function that makes no wave or block call
// is __host__ __device__ and written with plain operators, which under the build's -ffp-contract=off round every
// multiply and add separately as the __d*_rn forms do: tests/solve_dev_check.cpp runs those on the host.  A function
// with a barrier says so: every thread of the block calls it.
#pragma once
#include <stdint.h>

#include "thrl_device.h"

#include "thrl_chain_dev.h"      // chain_read_back; after the HIP declarations thrl_device.h brings

// on a lambda handed to these functions: inlined at every call, as the __forceinline__ functions around it are
#define THRL_SOLVE_INLINE __attribute__((always_inline))

namespace thrl {

namespace {

// the doubling rounds an evaluation needs: the smallest D with gam^(2^D) < 2^-64, at most 64
__host__ __device__ __forceinline__ int doubling_rounds(double gam) {
    int D = 0;
    for (double w = gam; w >= 0x1p-64 && D < 64; D++) w = w * w;
    return D;
}

// what V_pi gives up at a state, relative to V*
__host__ __device__ __forceinline__ double rel_loss(double vs, double vp) { return (vs == vp || vs == 0.0) ? 0.0 : (vs - vp) / vs; }

// an action replaces the incumbent of a Jacobi evaluation only when better by more than 2 gam^2 tol / (1 - gam)
__host__ __device__ __forceinline__ double improve_margin(double gam, double tol) { return (((2.0 * gam) * gam) * tol) / (1.0 - gam); }

// a reward under noise: q R + p NR
__host__ __device__ __forceinline__ double noise_blend(double q, double r, double p, double nr) { return q * r + p * nr; }

// the w of a band row of W entries from cell b0 whose cells b0 + w lie in [0, J): [band_first, band_end), at most J of
// them whatever W and b0 are (in int64, so that every b0 is defined)
__host__ __device__ __forceinline__ int band_first(int b0, int W) {
    const int64_t m = -(int64_t)b0;
    return b0 < 0 ? (int)(m < W ? m : W) : 0;
}
__host__ __device__ __forceinline__ int band_end(int b0, int W, int J) {
    const int64_t r = (int64_t)J - b0;
    return r <= 0 || W <= 0 ? 0 : (int)(r < W ? r : W);
}

// the first maximum of q(0) .. q(nact - 1) under strict >: the action, and its value in bv
template <typename Q>
__host__ __device__ __forceinline__ int first_max(int nact, Q q, double& bv) {
    int ba = 0;
    bv = q(0);
    for (int act = 1; act < nact; act++) {
        const double qv = q(act);
        if (qv > bv) { bv = qv; ba = act; }
    }
    return ba;
}

// The walk that marks first visits: from cur at step tm along next[], first[] = -1 wherever no walk has been.  At the
// first state met twice mu <- the step of its first visit and lam <- the steps since; returns that state, x_mu.  n + 1
// steps always reach it (mu and lam are left alone otherwise).  Lanes that walk the same words get the same result.
// (k_equilibrium keeps these lines inline, and improve_strict's: through the two functions its launch is 5 % slower.)
__host__ __device__ __forceinline__ int first_visit_walk(int16_t* first, const uint16_t* next, int n, int cur, int tm, int& mu, int& lam) {
    for (int guard = 0; guard <= n; guard++) {
        const int f = first[cur];
        if (f >= 0) { mu = f; lam = tm - f; break; }
        first[cur] = (int16_t)tm;
        cur = next[cur];
        tm++;
    }
    return cur;
}

// ------------------------------------------------------------------------------------------------ doubling, one element
// V' = V + w V o n, n' = n o n
__host__ __device__ __forceinline__ void double_value(const double* Vo, double* Vn, const uint16_t* no, uint16_t* nn, double w, int s) {
    const int m = no[s];
    Vn[s] = Vo[s] + w * Vo[m];
    nn[s] = no[m];
}

// p' = p o p, m' = min(m, m o p): the minimum over twice as many states of the orbit
__host__ __device__ __forceinline__ void double_min(const uint16_t* po, uint16_t* pn, const uint16_t* mo, uint16_t* mn, int s) {
    const int m = po[s];
    pn[s] = po[m];
    mn[s] = mo[s] < mo[m] ? mo[s] : mo[m];
}

// attractors in the order (basin, -rep); a key is never 0, since a basin holds its rep
__host__ __device__ __forceinline__ uint32_t attr_key(int basin, int s) { return ((uint32_t)basin << 16) | (uint32_t)(0xffff - s); }
__host__ __device__ __forceinline__ int attr_key_rep(uint32_t key) { return key ? 0xffff - (int)(key & 0xffffu) : -1; }

// ------------------------------------------------------------------------------------------------ staging the game
// One wave stages a game that starts at price st: pol <- the greedy action of every (agent, state) row and of x_0's N
// rows, entry(i, row) the action in agent i's table row; x0row <- x_0's rows; then put(s, t) for every state s, t the
// tuple of the greedy actions there.  Returns x_0's state, -1 if it is none, and t0 <- the tuple played at x_0.
// Contains a barrier, and the caller sets one before it reads what put() wrote.
template <typename A, typename Entry, typename Put>
__device__ __forceinline__ int stage_game(const A& a, double st, uint16_t* pol, int32_t* x0row, int lane, Entry entry, Put put, int& t0) {
    const int S = a.S, N = a.N;
    for (int e = lane; e < N * S + N; e += 64) {
        int i, row;
        if (e < N * S) {
            i = e / S;
            row = a.srow[e];
        } else {
            i = e - N * S;
            row = encode64_fast(st, a.ag[i]);
            x0row[i] = row;
        }
        pol[e] = (uint16_t)entry(i, row);
    }
    __syncthreads();
    int found = -1;
    for (int s = lane; s < S; s += 64) {
        int t = 0;
        bool eq = true;
        for (int i = 0; i < N; i++) {
            t += (int)pol[i * S + s] * a.tstride[i];
            eq = eq && a.srow[i * S + s] == x0row[i];
        }
        put(s, t);
        if (eq) found = s;
    }
    t0 = 0;
    for (int i = 0; i < N; i++) t0 += (int)pol[N * S + i] * a.tstride[i];
    const unsigned long long hit = __ballot(found >= 0);
    return hit ? __shfl(found, __ffsll((long long)hit) - 1) : -1;
}

// what agent i plays in its table row `row` under the policy words pg: the entry clamped to its action count
template <typename A>
__device__ __forceinline__ int row_action(const A& a, const uint16_t* __restrict__ pg, int i, int row) {
    return min((int)pg[a.row_off[i] + row], a.ag[i].n_actions - 1);
}

// the tuple the agents play in cell (or start) k of J, whose table rows are rows[i * J + k] clamped to the agent's rows
template <typename A>
__device__ __forceinline__ int cell_tuple(const A& a, const uint16_t* __restrict__ pg, const int32_t* __restrict__ rows, int J, int k) {
    int t = 0;
    for (int i = 0; i < a.N; i++) t += row_action(a, pg, i, clamp_row(rows[(int64_t)i * J + k], a.ag[i])) * a.tstride[i];
    return t;
}

// the tuple the agents other than `skip` (-1: every agent) play at tuple s of T, under the policy words pg [N][T]
template <typename A>
__device__ __forceinline__ int tuple_map(const A& a, const uint16_t* __restrict__ pg, int T, int s, int skip) {
    int t = 0;
    for (int j = 0; j < a.N; j++)
        if (j != skip) t += min((int)pg[j * T + s], a.n_actions[j] - 1) * a.tstride[j];
    return t;
}

// ------------------------------------------------------------------------------------------------ policy iteration
// V = the value of sigma by doubling, in LDS: V(s) = R(t) + gam V(succ(t)) at t = base[s] + sigma[s] * ts, D rounds over
// the ping-pong pairs (Va, Vb) and (na, nb).  Returns the buffer that holds V.  Contains barriers, the last one after
// the last write: every thread of the block of B calls it.
template <int B, typename Base, typename Succ>
__device__ __forceinline__ double* eval_doubling(double* Va, double* Vb, uint16_t* na, uint16_t* nb, const Base* base, const uint16_t* sigma,
                                                 int ts, const double* __restrict__ R, int n, int D, double gam, int tid, Succ succ) {
    double *Vo = Va, *Vn = Vb;
    uint16_t *no = na, *nn = nb;
    for (int s = tid; s < n; s += B) {
        const int t = (int)base[s] + (int)sigma[s] * ts;
        Vo[s] = R[t];
        no[s] = (uint16_t)succ(t);
    }
    __syncthreads();
    double w = gam;
    for (int d = 0; d < D; d++) {
        for (int s = tid; s < n; s += B) double_value(Vo, Vn, no, nn, w, s);
        __syncthreads();
        double* tv = Vo; Vo = Vn; Vn = tv;
        uint16_t* tn = no; no = nn; nn = tn;
        w = __dmul_rn(w, w);
    }
    return Vo;
}

// the strict improvement step: keep the incumbent unless some action is strictly better under V; whether this thread changed a state
template <int B, typename Base, typename Succ>
__device__ __forceinline__ bool improve_strict(const Base* base, uint16_t* sigma, int ts, int nact, const double* __restrict__ R,
                                               const double* V, int n, double gam, int tid, Succ succ) {
    bool changed = false;
    for (int s = tid; s < n; s += B) {
        const int b = base[s];
        const int tc = b + (int)sigma[s] * ts;
        const double qc = __dadd_rn(R[tc], __dmul_rn(gam, V[succ(tc)]));
        double bv;
        const int ba = first_max(nact, [&](int act) THRL_SOLVE_INLINE {
            const int t = b + act * ts;
            return __dadd_rn(R[t], __dmul_rn(gam, V[succ(t)]));
        }, bv);
        if (bv > qc) { sigma[s] = (uint16_t)ba; changed = true; }
    }
    return changed;
}

// ------------------------------------------------------------------------------------------------ outputs
// the wave's largest loss and its count of states whose best response differs
__device__ __forceinline__ void wave_max_sum(double& lmax, int& nd) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ol = __shfl_xor(lmax, m);
        if (ol > lmax) lmax = ol;
        nd += __shfl_xor(nd, m);
    }
}

// a state: the best response there, V* and V_pi
template <typename A>
__device__ __forceinline__ void store_state(const A& a, int64_t at, int br, double vs, double vp) {
    if (a.br_policy) a.br_policy[at] = (uint16_t)br;
    if (a.v_opt) a.v_opt[at] = vs;
    if (a.v_pi) a.v_pi[at] = vp;
}

// the n states from `at` of an agent or game that is not solved: v in both values, br(s) as the best response
template <typename A, typename Br>
__device__ __forceinline__ void store_states_unsolved(const A& a, int64_t at, int n, int lane, double v, Br br) {
    for (int s = lane; s < n; s += 64) store_state(a, at + s, br(s), v, v);
}

// an agent whose gamma lies outside [0, 1): NaN, one thread's stores
template <typename A>
__device__ __forceinline__ void store_agent_unsolved(const A& a, int64_t o) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    a.iters[o] = -1; a.n_diff_all[o] = 0; a.n_diff_on[o] = 0;
    a.loss_all[o] = nan; a.loss_on[o] = nan; a.loss_all_mean[o] = nan; a.loss_on_mean[o] = nan;
    a.v_on[o] = nan;
}

// the sums over the lam states of the cycle from c, in cycle order from 0.0; diff(c): 1 where the best response is not the agent's action
struct OnCycle { double sum, von, lon; int nd; };       // of the losses, of V_pi, the largest loss, the count
template <typename Diff>
__device__ __forceinline__ OnCycle on_cycle_sums(const double* loss, const double* Vpi, const uint16_t* jn, int c, int lam, Diff diff) {
    OnCycle r{0.0, 0.0, -__builtin_huge_val(), 0};
    for (int j = 0; j < lam; j++) {
        const double l = loss[c];
        r.sum = __dadd_rn(r.sum, l);
        r.von = __dadd_rn(r.von, Vpi[c]);
        if (l > r.lon) r.lon = l;
        r.nd += diff(c);
        c = jn[c];
    }
    return r;
}

// ------------------------------------------------------------------------------------------------ attractors
// one doubling round of the orbit minimum over n states, and the barrier after it: every thread of the block of B calls it
template <int B>
__device__ __forceinline__ void double_min_round(const uint16_t* po, uint16_t* pn, const uint16_t* mo, uint16_t* mn, int n, int tid) {
    for (int s = tid; s < n; s += B) double_min(po, pn, mo, mn, s);
    __syncthreads();
}

// one KEEP round's scan: the largest key below prev among this wave's attractors, 0 if none (the caller joins the waves)
template <int B>
__device__ __forceinline__ uint32_t keep_scan(const int32_t* basin, const uint16_t* rep, int n, uint32_t prev, int tid) {
    uint32_t best = 0;
    for (int s = tid; s < n; s += B) {
        const uint32_t key = attr_key(basin[s], s);
        if (rep[s] == s && key < prev && key > best) best = key;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, m));
    return best;
}

// slot k takes the attractor of the key: one thread's stores
__device__ __forceinline__ void keep_take(uint32_t best, int k, int32_t* sel, int16_t* slotof) {
    const int r = attr_key_rep(best);
    sel[k] = r;
    if (r >= 0) slotof[r] = (int16_t)k;
}

// The sums over a chunk of n start weights staged in LDS, in ascending order: threads 0 .. keep - 1 the weight that ends
// in their slot, thread keep the weight of the attractors not kept, the next N threads w * cycle_reward of their agent
// (rows of B terms).  The caller's barriers stand around it.
template <int B, typename Slot>
__device__ __forceinline__ double start_read_back(const Slot* cslot, const double* cw, const double* cprod, int keep, int N, int n, double acc, int tid) {
    if (tid > keep) return chain_read_back<B>(cprod, N, n, acc, tid - keep - 1);
    const int want = tid < keep ? tid : -1;
    for (int jj = 0; jj < n; jj++)
        if (cslot[jj] == want) acc = __dadd_rn(acc, cw[jj]);
    return acc;
}

// those sums of game g of G, keyed by thread as above
__device__ __forceinline__ void start_store(double* mass, double* other, double* reward, int64_t g, int64_t G, int keep, int N, int tid, double acc) {
    if (tid < keep) mass[(int64_t)tid * G + g] = acc;
    else if (tid == keep) other[g] = acc;
    else if (tid < keep + 1 + N) reward[(int64_t)(tid - keep - 1) * G + g] = acc;
}

}  // namespace

}  // namespace thrl
