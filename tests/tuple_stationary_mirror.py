"""numpy restatement of thrl_tuple_stationary (include/thrl.h) from given tuple_policy / cell_policy arrays and the
per-config tables of th_rl_amd.tuple_stationary.tables, written from the definitions: every sum runs in the stated
ascending order from 0.0 and every operation is rounded once.  Vectorised over games only: the loop over the source
tuples t of nu is explicit, and the segmented sums D, Nn and m_0 are numpy.add.at, which adds unbuffered, element by
element in index order (game-major, then ascending t or k)."""
import numpy as np

RESET = -2 ** 31        # analyse(): a start entry that asks for the reset distribution (the device has one flag per call)


def strides(n_actions):
    n = [int(x) for x in n_actions]
    return [int(np.prod(n[i + 1:])) for i in range(len(n))]


def tuple_of(tabs, pol):
    """[G, n]: the tuple index of the clamped entries of a uint16 strategy array [G, N, n]."""
    pol = np.asarray(pol).astype(np.int64)
    out = np.zeros((pol.shape[0], pol.shape[2]), np.int64)
    for i, (A, s) in enumerate(zip(tabs["n_actions"], strides(tabs["n_actions"]))):
        out += np.minimum(pol[:, i], int(A) - 1) * s
    return out


def ordered_sum(x):
    """Sum over the last axis in ascending order from 0.0."""
    s = np.zeros(x.shape[:-1])
    for k in range(x.shape[-1]):
        s = s + x[..., k]
    return s


def grouped(keys, values, T):
    """out[g, t'] = sum of values[g, j] over the j with keys[g, j] = t', in ascending j from 0.0."""
    out = np.zeros((keys.shape[0], T))
    rows = np.broadcast_to(np.arange(keys.shape[0])[:, None], keys.shape)
    np.add.at(out, (rows, keys), np.broadcast_to(values, keys.shape))
    return out


def switches(tabs, cell_policy, kinds=None):
    """n_switch int32 [G], unresolved [G]."""
    kinds = list(tabs["kinds"] if kinds is None else kinds)
    cp = np.asarray(cell_policy).astype(np.int64)
    G, _, J = cp.shape
    w = np.asarray(tabs["cell_w"], np.float64)
    flag = np.zeros((G, max(J - 1, 0)), bool)
    for i, k in enumerate(kinds):
        if k != "QTable":
            e = np.minimum(cp[:, i], int(tabs["n_actions"][i]) - 1)
            flag |= e[:, :-1] != e[:, 1:]
    un = np.zeros(G)
    for k in range(J - 1):
        un = np.where(flag[:, k], un + 0.5 * (w[k] + w[k + 1]), un)
    return flag.sum(axis=1).astype(np.int32), un


def step(tabs, F, tau, p, q, m):
    """One step of the chain for the games of m [G, T]: (m', chg)."""
    T, J, W = int(tabs["n_tuples"]), int(tabs["n_cells"]), int(tabs["band_w"])
    nu = np.zeros((m.shape[0], J))
    for t in range(T):
        lo = int(tabs["band_lo"][t])
        hi = min(lo + W, J)
        nu[:, lo:hi] = nu[:, lo:hi] + m[:, t:t + 1] * tabs["band"][t, :hi - lo][None, :]
    D = grouped(F, m, T)
    Nn = grouped(tau, nu, T)
    s = q[:, None] * D + p[:, None] * Nn
    new = 0.5 * m + 0.5 * s
    return new, np.abs(new - m).max(axis=1)


def analyse(tabs, tuple_policy, cell_policy, noise_prob, start=None, tol=1e-12, max_iters=8192, kinds=None):
    """Every output of thrl_tuple_stationary (pi, n_switch and unresolved included).  tuple_policy uint16 [G, N, T],
    cell_policy uint16 [G, N, J]; noise_prob a number or [G]; start int [G] = the start tuples of
    THRL_TS_START_TUPLE, None = the reset distribution; an entry RESET gives that game the reset distribution, so that
    the games of a call with the flag and of one without can be restated together."""
    T, N = int(tabs["n_tuples"]), len(tabs["n_actions"])
    F, tau = tuple_of(tabs, tuple_policy), tuple_of(tabs, cell_policy)
    G = F.shape[0]
    p = np.broadcast_to(np.asarray(noise_prob, np.float64), (G,)).copy()
    ok = (p > 0.0) & (p <= 1.0)
    m = grouped(tau, np.asarray(tabs["cell_w"], np.float64)[None, :], T)
    if start is not None:
        start = np.asarray(start, np.int64).reshape(G)
        unit = start != RESET
        ok &= ~unit | ((start >= 0) & (start < T))
        m[unit] = 0.0
        m[unit, np.clip(start[unit], 0, T - 1)] = 1.0
    pz = np.where(ok, p, 0.5)
    q = 1.0 - pz
    iters, change = np.zeros(G, np.int64), np.zeros(G)
    act = np.flatnonzero(ok)
    while act.size:
        new, chg = step(tabs, F[act], tau[act], pz[act], q[act], m[act])
        m[act] = new
        iters[act] += 1
        change[act] = chg
        act = act[~((chg <= tol) | (iters[act] >= max_iters))]
    rew = q[None, :, None] * tabs["reward"][:, None, :] + pz[None, :, None] * tabs["noise_reward"][:, None, :]
    price = q[:, None] * tabs["price"][None, :] + pz[:, None] * tabs["noise_price"][None, :]
    out = dict(iters=iters.astype(np.int32), change=change, mass=ordered_sum(m), stat_reward=ordered_sum(m[None] * rew),
               stat_action=ordered_sum(m[None] * tabs["scaled"][:, None, :]), stat_price=ordered_sum(m * price), pi=m)
    bad = ~ok
    out["iters"][bad] = -1
    for f in ("change", "mass", "stat_price"):
        out[f][bad] = 0.0
    out["pi"][bad] = 0.0
    out["stat_reward"][:, bad] = 0.0
    out["stat_action"][:, bad] = 0.0
    out["n_switch"], out["unresolved"] = switches(tabs, cell_policy, kinds)
    assert out["stat_reward"].shape == (N, G)
    return out
