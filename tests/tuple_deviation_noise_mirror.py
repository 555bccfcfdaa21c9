"""numpy restatement of the deviation test under demand noise in tuple form (thrl_tuple_deviation_noise, include/thrl.h),
written from its definitions on top of tuple_stationary_mirror (tuple_of, grouped, ordered_sum) and the per-config tables
of th_rl_amd.tuple_stationary.tables (the tables the device reads too).  analyse() is the recurrence itself, vectorised
over games, with an explicit ascending loop over the source tuples t of nu and numpy.add.at for the segmented sums D and
Nn (unbuffered, element by element in index order), so that every sum has the stated order and every operation is
rounded once: every output is reproducible to the bit.  dense() is a second, independent route for one game: the chains
on tuples as dense matrices and numpy's matrix products m_0 @ P'^min(tau, L) @ P^(tau - L), whose sums run in numpy's
order, not the definition's; dense_bound() is the rounding bound between the two.
"""
import numpy as np

import tuple_stationary_mirror as SM

FLOAT_FIELDS = ("dev_share", "gain", "gain_dev", "low", "dist", "mass")
INT_FIELDS = ("low_step", "ret_step")
AGENT_FIELDS = ("base_reward", "base_action")
ROW_FIELDS = ("reward_rows", "action_rows", "dist_rows")


def expected_rewards(tabs, p):
    """R_i(u) = q_g * reward_i(u) + p_g * noise_reward_i(u): [N, G, T]."""
    q = (1.0 - p)[None, :, None]
    return q * np.asarray(tabs["reward"])[:, None, :] + p[None, :, None] * np.asarray(tabs["noise_reward"])[:, None, :]


def deviation_map(tabs, R, deviator, dev_action):
    """Dv_g(t) int64 [G, T]: t with the deviator's action replaced by dev_action, or (-1) by the first maximum of R_d."""
    T = int(tabs["n_tuples"])
    ts, nA = SM.strides(tabs["n_actions"])[deviator], int(tabs["n_actions"][deviator])
    t = np.arange(T)
    t0 = t - ((t // ts) % nA) * ts
    G = R.shape[1]
    if dev_action >= 0:
        return np.broadcast_to(t0 + int(dev_action) * ts, (G, T)).copy()
    cand = np.stack([R[deviator][:, t0 + a * ts] for a in range(nA)], axis=-1)      # [G, T, A]
    return t0[None, :] + cand.argmax(axis=-1) * ts                                  # argmax: the first maximum


def full_band(tabs):
    """n(t, k) dense [T, J]; entries of a band row outside [0, J) are dropped."""
    T, J, W = int(tabs["n_tuples"]), int(tabs["n_cells"]), int(tabs["band_w"])
    n = np.zeros((T, J))
    for t in range(T):
        lo = int(tabs["band_lo"][t])
        for w in range(W):
            if 0 <= lo + w < J:
                n[t, lo + w] = tabs["band"][t, w]
    return n


def step(tabs, n, Fe, e, tau, p, q, m):
    """The plain step for the games of m [G, T]: e [G, T] the tuple played in place of t, Fe = F_g(e(t)) [G, T]."""
    T, J = int(tabs["n_tuples"]), int(tabs["n_cells"])
    nu = np.zeros((m.shape[0], J))
    for t in range(T):
        nu = nu + m[:, t:t + 1] * n[e[:, t]]
    D = SM.grouped(Fe, m, T)
    Nn = SM.grouped(tau, nu, T)
    return q[:, None] * D + p[:, None] * Nn


def analyse(tabs, tuple_policy, cell_policy, noise_prob, weights, deviator=0, steps=32, dev_len=1, dev_action=-1,
            ret_tol=1e-6, gamma=None, n_games=None):
    """Every output of thrl_tuple_deviation_noise, the rows for all tau < steps.  tuple_policy uint16 [G, N, T],
    cell_policy uint16 [G, N, J]; noise_prob a number or [G]; weights [G, T]; gamma [N] (one per agent) or [N, G]."""
    N, T = len(tabs["n_actions"]), int(tabs["n_tuples"])
    G = np.asarray(tuple_policy).shape[0] if n_games is None else int(n_games)
    K, L, d = int(steps), int(dev_len), int(deviator)
    p = np.broadcast_to(np.asarray(noise_prob, np.float64), (G,)).copy()
    with np.errstate(invalid="ignore"):
        ok = (p > 0.0) & (p <= 1.0)
    pz = np.where(ok, p, 0.5)
    q = 1.0 - pz
    gamma = np.asarray(gamma, np.float64)
    gam = np.full(G, float(gamma[d])) if gamma.ndim == 1 else gamma[d, :G]
    F = SM.tuple_of(tabs, np.asarray(tuple_policy)[:G])
    tau_k = SM.tuple_of(tabs, np.asarray(cell_policy)[:G])
    R = expected_rewards(tabs, pz)                                         # [N, G, T]
    sc = np.asarray(tabs["scaled"], np.float64)                            # [N, T]
    Dv = deviation_map(tabs, R, d, int(dev_action))
    ident = np.broadcast_to(np.arange(T), (G, T))
    FDv = np.take_along_axis(F, Dv, axis=1)
    n = full_band(tabs)
    m0 = np.array(np.asarray(weights, np.float64)[:G], copy=True)

    def sums(m, e, last):
        """[2N + 2, G]: E_i, A_i, the last sum (`last` [G, T] its terms) and the mass, each in ascending t."""
        terms = [m * np.take_along_axis(R[i], e, axis=1) for i in range(N)] + [m * sc[i][e] for i in range(N)]
        return SM.ordered_sum(np.stack(terms + [last, m]))

    base = sums(m0, ident, np.where(Dv != ident, m0, 0.0))
    out = dict(base_reward=base[:N].copy(), base_action=base[N:2 * N].copy(), dev_share=base[2 * N].copy())
    rr, ra, rd = np.zeros((K, N, G)), np.zeros((K, N, G)), np.zeros((K, G))
    w, gain, gain_dev, low = np.ones(G), np.zeros(G), np.zeros(G), np.zeros(G)
    low_step, ret = np.full(G, -1, np.int32), np.full(G, -1, np.int32)
    m = m0
    for t in range(K + 1):
        e, Fe = (Dv, FDv) if t < L else (ident, F)
        s = sums(m, e, np.abs(m - m0))
        D = 0.5 * s[2 * N]
        if t < K:
            rr[t], ra[t], rd[t] = s[:N], s[N:2 * N], D
            diff = s[d] - base[d]
            term = w * diff
            gain = gain + term
            if t < L:
                gain_dev = gain_dev + term
            else:
                lower = np.full(G, True) if t == L else diff < low
                low = np.where(lower, diff, low)
                low_step = np.where(lower, t, low_step).astype(np.int32)
            w = w * gam
        if t >= L:
            ret = np.where((ret < 0) & (D <= ret_tol), t, ret).astype(np.int32)
        if t == K:
            out.update(dist=D, mass=s[2 * N + 1].copy())
            break
        m = step(tabs, n, Fe, e, tau_k, pz, q, m)
    out.update(gain=gain, gain_dev=gain_dev, low=low, low_step=low_step, ret_step=ret, reward_rows=rr, action_rows=ra,
               dist_rows=rd)
    bad = ~ok
    for f in FLOAT_FIELDS:
        out[f][bad] = 0.0
    for f in INT_FIELDS:
        out[f][bad] = -1
    for f in AGENT_FIELDS + ROW_FIELDS:
        out[f][..., bad] = 0.0
    out.update(Dv=Dv, F=F, tau=tau_k, noise_prob=p)
    return out


# ---------------------------------------------------------------------------------------------- the dense route
def chain(tabs, n, Fe, e, tau_k, p):
    """One game's chain on tuples as a dense matrix [T, T]: P(t, t') = q [F(e(t)) = t'] + p sum over the k with tau(k) =
    t' of n(e(t), k), the inner sums in numpy's order."""
    T = int(tabs["n_tuples"])
    lump = np.zeros((n.shape[1], T))
    lump[np.arange(n.shape[1]), tau_k] = 1.0
    P = p * (n[e] @ lump)
    P[np.arange(T), Fe] += 1.0 - p
    return P


def dense(tabs, tuple_policy, cell_policy, noise_prob, weights, g, deviator=0, steps=32, dev_len=1, dev_action=-1):
    """E [K, N] of game g by dense products: M_0 = I, M_{tau+1} = M_tau @ P^(tau), m_tau = m_0 @ M_tau and E_i(tau) =
    m_tau @ R_i(e_tau), every sum in numpy's own order.  Also max |R|."""
    T = int(tabs["n_tuples"])
    G = np.asarray(tuple_policy).shape[0]
    p = np.broadcast_to(np.asarray(noise_prob, np.float64), (G,)).copy()
    F, tau_k = SM.tuple_of(tabs, tuple_policy), SM.tuple_of(tabs, cell_policy)
    R = expected_rewards(tabs, p)
    Dv = deviation_map(tabs, R, int(deviator), int(dev_action))
    n = full_band(tabs)
    ident = np.arange(T)
    P = chain(tabs, n, F[g], ident, tau_k[g], p[g])
    Pd = chain(tabs, n, F[g][Dv[g]], Dv[g], tau_k[g], p[g])
    m0 = np.asarray(weights, np.float64)[g]
    Mt = np.eye(T)
    Eo = np.zeros((int(steps), R.shape[0]))
    for t in range(int(steps)):
        e = Dv[g] if t < dev_len else ident
        Eo[t] = (m0 @ Mt) @ R[:, g, e].T
        Mt = Mt @ (Pd if t < dev_len else P)
    return Eo, float(np.abs(R[:, g]).max())


def dense_bound(tau, T, J, rmax):
    """The rounding bound between analyse() and dense() on E_i(tau), for a start distribution of mass at most 1.  One
    step forms a new entry from at most T products through nu, at most J adds in Nn and T adds in D, two products and
    one add: at most (T + J + 3) operations deep in either route, each with relative error 2^-53, on non-negative terms
    whose total is the mass, so a step moves the distribution by at most (T + J + 3) 2^-53 in either route and the two
    routes apart by twice that: (T + J + 3) 2^-52 per step in the 1-norm.  E then adds T products (T + 1 more operations
    in either route, the blend R itself two more), times max|R|.  Hence (tau (T + J + 3) + T + 3) 2^-52 max|R|, the form
    of deviation_noise_mirror.dense_bound with both index sets counted."""
    return (int(tau) * (T + J + 3) + T + 3) * 2.0 ** -52 * rmax
