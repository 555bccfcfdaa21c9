"""numpy restatement of the equilibrium check under demand noise in tuple form (thrl_tuple_equilibrium_noise,
include/thrl.h), written from its definitions on top of th_rl_amd.tuple_stationary.tables (the tables the device reads
too) and given tuple_policy / cell_policy arrays.  Vectorised over games with per-game "still sweeping" and "still
iterating" masks; the band sum is an explicit ascending loop over w, nu an explicit ascending loop over t and the output
sums explicit ascending loops over the states, so that every sum has the stated order and every operation is rounded
once.  Also the independent solvers the scheme is held against (the dense chain on the S = T + J states with
numpy.linalg.solve, plain value iteration) and the derived error bound.
"""
import numpy as np

import tuple_stationary_mirror as SM

MAX_ITERS = 64
INT_FIELDS = ("iters", "sweeps", "n_diff_tuples", "n_diff_cells")
FLOAT_FIELDS = ("loss_all", "loss_tuples_mean", "loss_cells_mean")
W_FIELDS = ("loss_w", "diff_w", "v_w")
STATE_FIELDS = ("br_policy", "v_opt", "v_pi")


def margin_of(gamma, eval_tol):
    """((2 * gamma) * gamma) * eval_tol / (1 - gamma), every operation rounded once."""
    gamma = np.asarray(gamma, np.float64)
    return ((2.0 * gamma) * gamma) * float(eval_tol) / (1.0 - gamma)


def state_tuples(tabs, tuple_policy, cell_policy):
    """[G, S]: the tuple played at every state, F_g(t) at the tuple-states, then tau_g(k) at the cells."""
    return np.concatenate([SM.tuple_of(tabs, tuple_policy), SM.tuple_of(tabs, cell_policy)], axis=1)


def losses(v_opt, v_pi):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((v_opt == v_pi) | (v_opt == 0.0), 0.0, (v_opt - v_pi) / v_opt)


def weights_of(tabs, pi, p):
    """w [G, S] from pi [G, T]: q * pi(t) at the tuple-states, p * nu(k) at the cells, nu(k) the sum over ascending t of
    pi(t) * band[t][k - band_lo[t]] over the t whose band holds k."""
    T, J, W = int(tabs["n_tuples"]), int(tabs["n_cells"]), int(tabs["band_w"])
    pi = np.asarray(pi, np.float64)
    p = np.asarray(p, np.float64)
    nu = np.zeros((pi.shape[0], J))
    for t in range(T):
        lo = int(tabs["band_lo"][t])
        k0, k1 = max(lo, 0), min(lo + W, J)
        if k1 > k0:
            nu[:, k0:k1] = nu[:, k0:k1] + pi[:, t:t + 1] * np.asarray(tabs["band"], np.float64)[t, k0 - lo:k1 - lo][None, :]
    return np.concatenate([(1.0 - p)[:, None] * pi, p[:, None] * nu], axis=1)


class Problem:
    """Agent i's problem in the games of tup [G, S]: the tuples t(s, a), R per tuple and x_V = R + gamma * z_V."""

    def __init__(self, tabs, tup, i, p, gamma):
        self.T, self.J, self.W = int(tabs["n_tuples"]), int(tabs["n_cells"]), int(tabs["band_w"])
        n_act = [int(x) for x in tabs["n_actions"]]
        self.A, ts = n_act[i], SM.strides(n_act)[i]
        self.p = np.asarray(p, np.float64)
        self.q = 1.0 - self.p
        self.gamma = np.asarray(gamma, np.float64)
        self.tup = tup
        self.pol = (tup // ts) % self.A                                          # pi_i(s) [G, S]
        self.tsa = (tup - self.pol * ts)[:, :, None] + np.arange(self.A)[None, None, :] * ts      # t(s, a) [G, S, A]
        self.ts = ts
        # R per tuple and game: q * reward_i(t) + p * noise_reward_i(t)
        self.Rt = self.q[:, None] * np.asarray(tabs["reward"], np.float64)[i][None, :] \
            + self.p[:, None] * np.asarray(tabs["noise_reward"], np.float64)[i][None, :]
        c = np.asarray(tabs["band_lo"], np.int64)[:, None] + np.arange(self.W)[None, :]            # [T, W]
        self.ok = (c >= 0) & (c < self.J)
        self.cell = np.clip(c, 0, self.J - 1)
        # a term whose cell lies outside [0, J) becomes +0.0 and is added: b + 0.0 == b bit for bit (b is never -0.0),
        # which is skipping it
        self.band = np.where(self.ok, np.asarray(tabs["band"], np.float64), 0.0)

    def x(self, V, gs):
        """R(t) + gamma * z_V(t) for every tuple of the games gs: V [n, S] -> [n, T]."""
        T = self.T
        VJ = V[:, T:]
        terms = self.band[None, :, :] * VJ[:, self.cell]                         # [n, T, W]
        if not self.ok.all():
            terms = np.where(self.ok[None], terms, 0.0)
        b = np.zeros((V.shape[0], T))
        for w in range(self.W):
            b = b + terms[:, :, w]
        z = self.q[gs][:, None] * V[:, :T] + self.p[gs][:, None] * b
        return self.Rt[gs] + self.gamma[gs][:, None] * z

    def evaluate(self, V, tcur, gs, eval_tol, max_sweeps):
        """Jacobi from V [n, S] for the strategies' tuples tcur [n, S] of the games gs: (V, sweeps [n], capped [n])."""
        n = len(gs)
        V = V.copy()
        sweeps, capped = np.zeros(n, np.int64), np.zeros(n, bool)
        act = np.arange(n)
        while act.size:
            x = self.x(V[act], gs[act])
            new = np.take_along_axis(x, tcur[act], axis=1)
            chg = np.abs(new - V[act]).max(axis=1)
            V[act] = new
            sweeps[act] += 1
            done = chg <= eval_tol
            cap = ~done & (sweeps[act] >= max_sweeps)
            capped[act[cap]] = True
            act = act[~(done | cap)]
        return V, sweeps, capped


def analyse(tabs, tuple_policy, cell_policy, noise_prob, agents=None, gamma=None, eval_tol=1e-12, max_sweeps=8192,
            pi=None, n_games=None):
    """Every output of thrl_tuple_equilibrium_noise, with the per-state arrays.  tuple_policy uint16 [G, N, T],
    cell_policy uint16 [G, N, J]; noise_prob a number or [G]; gamma [N] per agent or [N, G] per game; pi [G, T] or
    None."""
    T, J = int(tabs["n_tuples"]), int(tabs["n_cells"])
    N, S = len(tabs["n_actions"]), T + J
    G = np.asarray(tuple_policy).shape[0] if n_games is None else int(n_games)
    agents = list(range(N)) if agents is None else sorted(agents)
    p = np.broadcast_to(np.asarray(noise_prob, np.float64), (G,)).copy()
    okp = (p > 0.0) & (p <= 1.0)
    pz = np.where(okp, p, 0.5)
    tup = state_tuples(tabs, np.asarray(tuple_policy)[:G], np.asarray(cell_policy)[:G])
    gamma = np.asarray(gamma, np.float64)
    gamma = np.repeat(gamma[:, None], G, axis=1) if gamma.ndim == 1 else gamma[:, :G]
    out = {f: np.zeros((N, G), np.int32) for f in INT_FIELDS}
    out.update({f: np.zeros((N, G)) for f in FLOAT_FIELDS + (W_FIELDS if pi is not None else ())})
    out["br_policy"] = np.zeros((N, G, S), np.uint16)
    out["v_opt"], out["v_pi"] = np.zeros((N, G, S)), np.zeros((N, G, S))
    wts = None if pi is None else weights_of(tabs, np.asarray(pi, np.float64)[:G], pz)
    ar = np.arange(S)[None, :]
    for i in agents:
        gam = gamma[i]
        okg = (gam >= 0.0) & (gam < 1.0)
        pr = Problem(tabs, tup, i, pz, np.where(okg, gam, 0.0))
        margin = margin_of(np.where(okg, gam, 0.0), eval_tol)
        tcur = tup.copy()
        V = np.zeros((G, S))
        v_pi = np.zeros((G, S))
        iters = np.full(G, -1, np.int64)
        sweeps = np.zeros(G, np.int64)
        capped = np.zeros(G, bool)
        live = np.flatnonzero(okp & okg)
        n = 0
        while live.size:
            Vl, sw, cap = pr.evaluate(V[live], tcur[live], live, eval_tol, max_sweeps)
            V[live] = Vl
            sweeps[live] += sw
            capped[live[cap]] = True
            live = live[~cap]
            if n == 0:
                v_pi[live] = V[live]
            if n == MAX_ITERS:
                capped[live] = True
                break
            if not live.size:
                break
            x = pr.x(V[live], live)
            rows = np.arange(live.size)[:, None]
            Q = x[rows[:, :, None], pr.tsa[live]]                                # Q(s, a) = x(t(s, a)) [n, S, A]
            best = np.argmax(Q, axis=2)                                          # first maximum
            better = Q[rows, ar, best] > x[rows, tcur[live]] + margin[live][:, None]
            tcur[live] = np.where(better, pr.tsa[live][rows, ar, best], tcur[live])
            stop = ~better.any(axis=1)
            iters[live[stop]] = n
            live = live[~stop]
            n += 1
        solved = okp & okg & ~capped
        loss = losses(V, v_pi)
        diff = tcur != tup
        nan = np.where(solved, 0.0, np.nan)
        out["iters"][i] = np.where(solved, iters, -1)
        out["sweeps"][i] = sweeps
        out["n_diff_tuples"][i] = np.where(solved, diff[:, :T].sum(axis=1), 0)
        out["n_diff_cells"][i] = np.where(solved, diff[:, T:].sum(axis=1), 0)
        out["loss_all"][i] = loss.max(axis=1) + nan
        out["loss_tuples_mean"][i] = SM.ordered_sum(loss[:, :T]) / float(T) + nan
        out["loss_cells_mean"][i] = SM.ordered_sum(loss[:, T:]) / float(J) + nan
        if wts is not None:
            out["loss_w"][i] = SM.ordered_sum(wts * loss) + nan
            out["diff_w"][i] = SM.ordered_sum(np.where(diff, wts, 0.0)) + nan
            out["v_w"][i] = SM.ordered_sum(wts * v_pi) + nan
        out["br_policy"][i] = np.where(solved[:, None], (tcur // pr.ts) % pr.A, pr.pol)
        out["v_opt"][i] = V + nan[:, None]
        out["v_pi"][i] = v_pi + nan[:, None]
        bad = ~okp                                                               # a bad noise probability: zeros
        for f in out:
            out[f][i][bad] = -1 if f == "iters" else 0
    out["n_cells"], out["T"] = J, T
    return out


# ---------------------------------------------------------------------------------------------- independent solvers
def full_band(tabs):
    """n [T, J]: the band table as the dense matrix n(t, k)."""
    T, J, W = int(tabs["n_tuples"]), int(tabs["n_cells"]), int(tabs["band_w"])
    n = np.zeros((T, J))
    for t in range(T):
        lo = int(tabs["band_lo"][t])
        for w in range(W):
            if 0 <= lo + w < J:
                n[t, lo + w] = tabs["band"][t, w]
    return n


def dense(tabs, tup, i, p):
    """Agent i's problem in one game as dense arrays over the S states: R [S, A], P [S, A, S] and pi_i [S] (tup [S], p
    a number).  After tuple t the next state is tuple-state t with probability q, cell-state k with p * n(t, k)."""
    T, J = int(tabs["n_tuples"]), int(tabs["n_cells"])
    n_act = [int(x) for x in tabs["n_actions"]]
    A, ts = n_act[i], SM.strides(n_act)[i]
    q = 1.0 - p
    pol = (tup // ts) % A
    tsa = (tup - pol * ts)[:, None] + np.arange(A)[None, :] * ts
    R = q * np.asarray(tabs["reward"])[i][tsa] + p * np.asarray(tabs["noise_reward"])[i][tsa]
    Pt = np.concatenate([q * np.eye(T), p * full_band(tabs)], axis=1)            # [T, S] by the tuple played
    return R, Pt[tsa], pol


def direct_value(R, P, sigma, gamma):
    """V_sigma = (I - gamma P_sigma)^-1 R_sigma."""
    ar = np.arange(R.shape[0])
    return np.linalg.solve(np.eye(R.shape[0]) - gamma * P[ar, sigma], R[ar, sigma])


def value_iteration(R, P, gamma, n=None):
    """Plain value iteration from 0, far past convergence: n sweeps with gamma^n < 2^-64 (or the n given)."""
    if n is None:
        w, n = 1.0, 0
        while w >= 2.0 ** -64:
            w *= float(gamma)
            n += 1
    V = np.zeros(R.shape[0])
    for _ in range(n):
        V = (R + gamma * (P @ V)).max(axis=1)
    return V


def error_bound(gamma, eval_tol, W, vmax):
    """How far a stopped evaluation may be from the strategy's true value.  Truncation: successive iterates within
    eval_tol and a contraction with factor gamma leave gamma / (1 - gamma) * eval_tol.  Rounding: a sweep computes a
    state's value in W multiplies and W adds of the band sum, the multiplies by p, q and gamma, the add of the q term and
    the add of the reward; the band weights are nonnegative and sum to at most 1, so each of the W + 3 roundings a value
    passes through on its longest path is relative u = 2^-53 of a quantity no larger than max|V|, and the computed sweep
    differs from the exact sweep of the same iterate by at most (W + 3) u max|V|.  The number of states S does not
    enter: a state's value is read back from its tuple's, not summed over states.  The fixed point of the perturbed sweep
    is within that amplified by 1 / (1 - gamma)."""
    return gamma / (1.0 - gamma) * eval_tol + (W + 3) * 2.0 ** -53 * vmax / (1.0 - gamma)
