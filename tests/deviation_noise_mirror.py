"""numpy restatement of the deviation test under demand noise (thrl_deviation_noise, include/thrl.h), written from its
definitions on top of stationary_mirror (cell_tuples, chain, values, ordered_sum), th_rl_amd.stationary.tables (the tables
the device reads too) and equilibrium_mirror's plan (the noise-free rewards).  analyse() is the recurrence itself,
vectorised over games, with an explicit ascending loop over the source cells j so that every sum has the stated order
and every operation is rounded once: every output is reproducible to the bit.  dense() is a second, independent route
for one game: the chains as dense matrices and numpy's matrix products m_0 @ P'^min(tau, L) @ P^(tau - L), whose sums
run in numpy's order, not the definition's; dense_bound() is the rounding bound between the two.
"""
import numpy as np

import deviation_mirror as M
import equilibrium_mirror as E
import stationary_mirror as S

FLOAT_FIELDS = ("dev_share", "gain", "gain_dev", "low", "dist", "mass")
INT_FIELDS = ("low_step", "ret_step")
AGENT_FIELDS = ("base_reward", "base_action")
ROW_FIELDS = ("reward_rows", "action_rows", "dist_rows")


def scaled(config):
    """sc_i(t) [N, T]: the scaled action of agent i in tuple t."""
    pl = E.plan(config)
    idx = np.unravel_index(np.arange(pl["T"]), pl["n_actions"])
    return np.stack([M.scale(idx[i], pl["ag"][i]) for i in range(pl["N"])])


def expected_rewards(config, tabs, p):
    """R_i(t) = q_g * r_i(t) + p_g * noise_reward_i(t): [N, G, T]."""
    pl = E.plan(config)
    q = (1.0 - p)[:, None]
    return np.stack([q * pl["rew"][i][None, :] + p[:, None] * tabs["noise_reward"][i][None, :] for i in range(pl["N"])])


def deviation_tuples(config, tup, R, deviator, dev_action):
    """t'_g(k) [G, J]: tup with the deviator's action replaced by dev_action, or (-1) by the first maximum of R_d."""
    pl = E.plan(config)
    ts, nA = int(pl["tstride"][deviator]), int(pl["n_actions"][deviator])
    cur = (tup // ts) % nA
    t0 = tup - cur * ts
    if dev_action >= 0:
        return t0 + int(dev_action) * ts
    cand = np.stack([np.take_along_axis(R[deviator], t0 + a * ts, axis=1) for a in range(nA)], axis=-1)    # [G, J, A]
    return t0 + cand.argmax(axis=-1) * ts                                  # argmax: the first maximum


def analyse(config, tabs, policy, noise_prob, weights, deviator=0, steps=32, dev_len=1, dev_action=-1, ret_tol=1e-6,
            gamma=None, n_games=None):
    """Every output of thrl_deviation_noise, the rows for all tau < steps.  policy [G, P]; noise_prob a number or [G];
    weights [G, J]; gamma [N, G] = the sweep's, None = the config's."""
    pl = E.plan(config)
    N, J = pl["N"], tabs["n_cells"]
    G = np.asarray(policy).shape[0] if n_games is None else int(n_games)
    K, L, d = int(steps), int(dev_len), int(deviator)
    p = np.broadcast_to(np.asarray(noise_prob, np.float64), (G,)).copy()
    with np.errstate(invalid="ignore"):
        ok = (p > 0.0) & (p <= 1.0)
    pz = np.where(ok, p, 0.5)
    q = 1.0 - pz
    gam = np.full(G, float(pl["ag"][d]["gamma"])) if gamma is None else np.asarray(gamma, np.float64)[d, :G]
    tup = S.cell_tuples(config, policy, tabs, G)
    R = expected_rewards(config, tabs, pz)                                 # [N, G, T]
    sc = scaled(config)                                                    # [N, T]
    tupd = deviation_tuples(config, tup, R, d, int(dev_action))
    n = S.full_band(tabs)
    det_cell = np.asarray(tabs["det_cell"], np.int64)
    cells = np.arange(J)[None, :]
    m0 = np.array(np.asarray(weights, np.float64)[:G], copy=True)

    def sums(m, tc, last):
        """[2N + 2, G]: E_i, A_i, the last sum (`last` [G, J] its terms) and the mass, each in ascending k."""
        terms = [m * np.take_along_axis(R[i], tc, axis=1) for i in range(N)] + [m * sc[i][tc] for i in range(N)]
        return S.ordered_sum(np.stack(terms + [last, m]))

    def step(m, tc):
        s = np.zeros_like(m)
        det = det_cell[tc]
        for j in range(J):
            Pj = pz[:, None] * n[tc[:, j]]
            Pj = np.where(det[:, j][:, None] == cells, q[:, None] + Pj, Pj)
            s = s + m[:, j:j + 1] * Pj
        return s

    base = sums(m0, tup, np.where(tupd != tup, m0, 0.0))
    out = dict(base_reward=base[:N].copy(), base_action=base[N:2 * N].copy(), dev_share=base[2 * N].copy())
    rr, ra, rd = np.zeros((K, N, G)), np.zeros((K, N, G)), np.zeros((K, G))
    w, gain, gain_dev, low = np.ones(G), np.zeros(G), np.zeros(G), np.zeros(G)
    low_step, ret = np.full(G, -1, np.int32), np.full(G, -1, np.int32)
    m = m0
    for tau in range(K + 1):
        tc = tupd if tau < L else tup
        s = sums(m, tc, np.abs(m - m0))
        D = 0.5 * s[2 * N]
        if tau < K:
            rr[tau], ra[tau], rd[tau] = s[:N], s[N:2 * N], D
            diff = s[d] - base[d]
            term = w * diff
            gain = gain + term
            if tau < L:
                gain_dev = gain_dev + term
            else:
                lower = np.full(G, True) if tau == L else diff < low
                low = np.where(lower, diff, low)
                low_step = np.where(lower, tau, low_step).astype(np.int32)
            w = w * gam
        if tau >= L:
            ret = np.where((ret < 0) & (D <= ret_tol), tau, ret).astype(np.int32)
        if tau == K:
            out.update(dist=D, mass=s[2 * N + 1].copy())
            break
        m = step(m, tc)
    out.update(gain=gain, gain_dev=gain_dev, low=low, low_step=low_step, ret_step=ret, reward_rows=rr, action_rows=ra,
               dist_rows=rd)
    bad = ~ok
    for f in FLOAT_FIELDS:
        out[f][bad] = 0.0
    for f in INT_FIELDS:
        out[f][bad] = -1
    for f in AGENT_FIELDS + ROW_FIELDS:
        out[f][..., bad] = 0.0
    out.update(tup=tup, tupd=tupd, noise_prob=p)
    return out


# ---------------------------------------------------------------------------------------------- the dense route
def dense(config, tabs, policy, noise_prob, weights, g, deviator=0, steps=32, dev_len=1, dev_action=-1):
    """E [K, N] of game g by dense products: M_0 = I, M_{tau+1} = M_tau @ P^(tau), m_tau = m_0 @ M_tau and E_i(tau) =
    m_tau @ R_i(t^(tau)), every sum in numpy's own order.  Also max |R|."""
    pl = E.plan(config)
    G = np.asarray(policy).shape[0]
    p = np.broadcast_to(np.asarray(noise_prob, np.float64), (G,)).copy()
    tup = S.cell_tuples(config, policy, tabs, G)
    R = expected_rewards(config, tabs, p)
    tupd = deviation_tuples(config, tup, R, int(deviator), int(dev_action))
    P, Pd = S.chain(tabs, tup[g], p[g]), S.chain(tabs, tupd[g], p[g])
    m0 = np.asarray(weights, np.float64)[g]
    Mt = np.eye(tabs["n_cells"])
    Eo = np.zeros((int(steps), pl["N"]))
    for tau in range(int(steps)):
        tc = tupd[g] if tau < dev_len else tup[g]
        Eo[tau] = (m0 @ Mt) @ R[:, g, tc].T
        Mt = Mt @ (Pd if tau < dev_len else P)
    return Eo, float(np.abs(R[:, g]).max())


def dense_bound(tau, J, rmax):
    """The rounding bound between analyse() and dense() on E_i(tau), for a start distribution of mass at most 1: every
    step adds at most J products per cell, so after tau steps the two routes are within tau * (J + 2) * 2^-52 * max|R|,
    the form of test_gpu_stationary._identity.  The sum E itself adds J products once more in either route, which that
    form does not count; at tau = 0, where it gives 0, this one term (J + 2) * 2^-52 * max|R| is the bound."""
    return max(int(tau), 1) * (J + 2) * 2.0 ** -52 * rmax
