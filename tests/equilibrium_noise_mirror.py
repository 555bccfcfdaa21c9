"""numpy restatement of the equilibrium check under demand noise (thrl_equilibrium_noise, include/thrl.h), written
from its definitions on top of th_rl_amd.stationary.tables (the tables the device reads too), stationary_mirror's cell
tuples and equilibrium_mirror's plan (the noise-free rewards).  Vectorised over games with per-game "still sweeping" and
"still iterating" masks; the band sum is an explicit ascending loop over w and the output sums explicit ascending loops
over k, so that every sum has the stated order and every operation is rounded once.  Also the independent solvers the
scheme is held against (the dense chain with numpy.linalg.solve, plain value iteration) and the hand-built strategies
of the known answers.
"""
import numpy as np

import equilibrium_mirror as E
import stationary_mirror as S

MAX_ITERS = 64
INT_FIELDS = ("iters", "sweeps", "n_diff_all")
FLOAT_FIELDS = ("loss_all", "loss_all_mean")
W_FIELDS = ("loss_w", "diff_w", "v_w")
CELL_FIELDS = ("br_policy", "v_opt", "v_pi")


def margin_of(gamma, eval_tol):
    """((2 * gamma) * gamma) * eval_tol / (1 - gamma), every operation rounded once."""
    gamma = np.asarray(gamma, np.float64)
    return ((2.0 * gamma) * gamma) * float(eval_tol) / (1.0 - gamma)


class Problem:
    """Agent i's problem in the games `gs` (indices into tup's rows): the tuples t(k, a), R(k, a) and z_V."""

    def __init__(self, pl, tabs, tup, i, p, gamma):
        self.J, self.W, self.T = int(tabs["n_cells"]), int(tabs["band_w"]), int(tabs["n_tuples"])
        self.A, ts = pl["n_actions"][i], pl["tstride"][i]
        self.p = np.asarray(p, np.float64)
        self.q = 1.0 - self.p
        self.gamma = np.asarray(gamma, np.float64)
        self.pol = (tup // ts) % self.A                                          # pi_i(k) [G, J]
        self.tka = (tup - self.pol * ts)[:, :, None] + np.arange(self.A)[None, None, :] * ts      # t(k, a) [G, J, A]
        # R per tuple and game: q * r_i(t) + p * noise_reward_i(t)
        self.Rt = self.q[:, None] * pl["rew"][i][None, :] + self.p[:, None] * np.asarray(tabs["noise_reward"][i])[None, :]
        self.det = np.asarray(tabs["det_cell"], np.int64)
        self.blo = np.asarray(tabs["band_lo"], np.int64)
        self.band = np.asarray(tabs["band"], np.float64)

    def z(self, V, t, gs):
        """z_V(t) for the games gs: V [n, J], t [n, ...] tuples -> [n, ...]."""
        J = self.J
        sh = (len(gs),) + (1,) * (t.ndim - 1)
        rows = np.arange(len(gs)).reshape(sh)
        q, p = self.q[gs].reshape(sh), self.p[gs].reshape(sh)
        d = self.det[t]
        inside = (d >= 0) & (d < J)
        s0 = np.where(inside, q * V[rows, np.clip(d, 0, J - 1)], 0.0)
        b = np.zeros(t.shape)
        for w in range(self.W):
            c = self.blo[t] + w
            ok = (c >= 0) & (c < J)
            b = np.where(ok, b + self.band[t, w] * V[rows, np.clip(c, 0, J - 1)], b)
        return s0 + p * b

    def evaluate(self, V, sigma, gs, eval_tol, max_sweeps):
        """Jacobi from V [n, J] for the strategies sigma [n, J] of the games gs: (V, sweeps [n], capped [n])."""
        n = len(gs)
        V = V.copy()
        sweeps, capped = np.zeros(n, np.int64), np.zeros(n, bool)
        ar = np.arange(self.J)[None, :]
        t_all = self.tka[gs[:, None], ar, sigma]                                 # [n, J]
        R_all = self.Rt[gs[:, None], t_all]
        act = np.arange(n)
        while act.size:
            g = gs[act]
            t = t_all[act]
            # the gathers do not change from sweep to sweep: kept while the set of sweeping games stays the same.  A term
            # whose cell lies outside [0, J) is replaced by +0.0 and added: b + 0.0 == b bit for bit, which is skipping it
            n_act = act.size
            d = self.det[t]
            inside = (d >= 0) & (d < self.J)
            flat0 = (np.arange(n_act)[:, None] * self.J)
            dflat = (flat0 + np.clip(d, 0, self.J - 1)).ravel()
            c = self.blo[t][None, :, :] + np.arange(self.W)[:, None, None]                  # [W, n, J]
            ok = (c >= 0) & (c < self.J)
            cflat = (flat0[None, :, :] + np.clip(c, 0, self.J - 1)).ravel()
            bw = np.where(ok, np.moveaxis(self.band[t], 2, 0), 0.0)                         # band[t][w], [W, n, J]
            skip = not bool(ok.all())
            q, p, gam = self.q[g][:, None], self.p[g][:, None], self.gamma[g][:, None]
            R = R_all[act]
            while True:
                Vo = V[act]
                vf = Vo.ravel()
                s0 = np.where(inside, q * vf.take(dflat).reshape(t.shape), 0.0)
                terms = bw * vf.take(cflat).reshape(bw.shape)
                if skip:
                    terms = np.where(ok, terms, 0.0)
                b = np.zeros(t.shape)
                for w in range(self.W):
                    b = b + terms[w]
                new = R + gam * (s0 + p * b)
                chg = np.abs(new - Vo).max(axis=1)
                V[act] = new
                sweeps[act] += 1
                done = chg <= eval_tol
                cap = ~done & (sweeps[act] >= max_sweeps)
                capped[act[cap]] = True
                if (done | cap).any():
                    act = act[~(done | cap)]
                    break
        return V, sweeps, capped


def _ordered(x):
    return S.ordered_sum(x)


def analyse(config, tabs, policy, noise_prob, agents=None, gamma=None, eval_tol=1e-12, max_sweeps=8192, weights=None,
            n_games=None):
    """Every output of thrl_equilibrium_noise, with the per-cell arrays.  policy [G, P]; noise_prob a number or [G];
    gamma [N, G] per game (a sweep) or None; weights [G, J] or None."""
    pl = E.plan(config)
    N, J = pl["N"], int(tabs["n_cells"])
    G = np.asarray(policy).shape[0] if n_games is None else int(n_games)
    agents = list(range(N)) if agents is None else sorted(agents)
    p = np.broadcast_to(np.asarray(noise_prob, np.float64), (G,)).copy()
    okp = (p > 0.0) & (p <= 1.0)
    pz = np.where(okp, p, 0.5)
    tup = S.cell_tuples(config, policy, tabs, G)
    out = {f: np.zeros((N, G), np.int32) for f in INT_FIELDS}
    out.update({f: np.zeros((N, G)) for f in FLOAT_FIELDS + (W_FIELDS if weights is not None else ())})
    out["br_policy"] = np.zeros((N, G, J), np.uint16)
    out["v_opt"], out["v_pi"] = np.zeros((N, G, J)), np.zeros((N, G, J))
    wts = None if weights is None else np.asarray(weights, np.float64)[:G]
    for i in agents:
        gam = np.asarray(gamma, np.float64)[i][:G] if gamma is not None else np.full(G, float(pl["ag"][i]["gamma"]))
        okg = (gam >= 0.0) & (gam < 1.0)
        pr = Problem(pl, tabs, tup, i, pz, np.where(okg, gam, 0.0))
        margin = margin_of(np.where(okg, gam, 0.0), eval_tol)
        ar = np.arange(J)[None, :]
        sigma = pr.pol.copy()
        V = np.zeros((G, J))
        v_pi = np.zeros((G, J))
        iters = np.full(G, -1, np.int64)
        sweeps = np.zeros(G, np.int64)
        capped = np.zeros(G, bool)
        live = np.flatnonzero(okp & okg)
        n = 0
        while live.size:
            Vl, sw, cap = pr.evaluate(V[live], sigma[live], live, eval_tol, max_sweeps)
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
            Q = pr.Rt[live[:, None, None], pr.tka[live]] + pr.gamma[live][:, None, None] * pr.z(V[live], pr.tka[live], live)
            best = np.argmax(Q, axis=2)                                          # first maximum
            rows = np.arange(live.size)[:, None]
            better = Q[rows, ar, best] > Q[rows, ar, sigma[live]] + margin[live][:, None]
            sigma[live] = np.where(better, best, sigma[live])
            stop = ~better.any(axis=1)
            iters[live[stop]] = n
            live = live[~stop]
            n += 1
        solved = okp & okg & ~capped
        loss = E.losses(V, v_pi)
        diff = sigma != pr.pol
        nan = np.where(solved, 0.0, np.nan)
        out["iters"][i] = np.where(solved, iters, -1)
        out["sweeps"][i] = sweeps
        out["n_diff_all"][i] = np.where(solved, diff.sum(axis=1), 0)
        out["loss_all"][i] = loss.max(axis=1) + nan
        out["loss_all_mean"][i] = _ordered(loss) / float(J) + nan
        if wts is not None:
            out["loss_w"][i] = _ordered(wts * loss) + nan
            out["diff_w"][i] = _ordered(np.where(diff, wts, 0.0)) + nan
            out["v_w"][i] = _ordered(wts * v_pi) + nan
        out["br_policy"][i] = np.where(solved[:, None], sigma, pr.pol)
        out["v_opt"][i] = V + nan[:, None]
        out["v_pi"][i] = v_pi + nan[:, None]
        bad = ~okp                                                               # a bad noise probability: zeros
        for f in out:
            out[f][i][bad] = -1 if f == "iters" else 0
    out["n_cells"] = J
    return out


# ---------------------------------------------------------------------------------------------- independent solvers
def dense(pl, tabs, tup, i, p):
    """Agent i's problem in one game as dense arrays: R [J, A] and P [J, A, J] from S.full_band (tup [J], p a number)."""
    J, A, ts = int(tabs["n_cells"]), pl["n_actions"][i], pl["tstride"][i]
    nb = S.full_band(tabs)
    q = 1.0 - p
    pol = (tup // ts) % A
    tka = (tup - pol * ts)[:, None] + np.arange(A)[None, :] * ts
    R = q * pl["rew"][i][tka] + p * np.asarray(tabs["noise_reward"][i])[tka]
    P = p * nb[tka]                                                              # [J, A, J]
    det = np.asarray(tabs["det_cell"])[tka]
    for k in range(J):
        for a in range(A):
            if 0 <= det[k, a] < J:
                P[k, a, det[k, a]] += q
    return R, P, pol


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
    cell's value in W multiplies and W adds of the band sum, the multiplies by p, q and gamma, the add of the q term and
    the add of the reward; as a rounding-error analysis of that dot product of nonnegative weights summing to at most 1
    the computed value differs from the exact sweep of the same iterate by at most (W + 3) u max|V| with u = 2^-53
    (each of the W + 3 roundings a value passes through on its longest path is relative u of a quantity no larger than
    max|V|).  The fixed point of the perturbed sweep is within that amplified by 1 / (1 - gamma)."""
    return gamma / (1.0 - gamma) * eval_tol + (W + 3) * 2.0 ** -53 * vmax / (1.0 - gamma)


constant_tables = E.strategy_tables
policies = S.policies
fresh_tables = S.fresh_tables
