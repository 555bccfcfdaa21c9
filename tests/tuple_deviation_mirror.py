"""numpy restatement of thrl_tuple_deviation (include/thrl.h) from a given tuple_policy array and tuple_play.tables():
a plain first-repeat cycle search (not the kernel's Brent search), the same sums in the same order."""
import numpy as np


def greedy_map(tabs, policy_g):
    """F [T] of one game: the index of the tuple (pi_i(t))_i, entries clamped to the last action, agent 0 slowest."""
    f = np.zeros(policy_g.shape[1], np.int64)
    for i, A in enumerate(int(a) for a in tabs["n_actions"]):
        f = f * A + np.minimum(policy_g[i].astype(np.int64), A - 1)
    return f


def cycle(F, t0, H):
    """(mu, lam, s*) of the path from t0 under the horizon rule: found iff mu + lam <= H, else (H, 0, t_H)."""
    seen, t = {int(t0): 0}, int(t0)
    for k in range(1, H + 1):
        t = int(F[t])
        if t in seen:
            return seen[t], k - seen[t], t
        seen[t] = k
    return H, 0, t


def analyse(tabs, policy, start, deviator=0, steps=32, dev_len=1, action=-1, horizon=None, gamma=0.95):
    """Every output of thrl_tuple_deviation for all games; the rows [steps, N, G] in full.  action: an index, or -1 =
    best response.  gamma: the deviator's discount, a number or [G]."""
    from th_rl_amd.deviation import default_horizon
    policy = np.asarray(policy)
    policy = policy.view(np.uint16) if policy.dtype == np.int16 else policy
    start = np.asarray(start, np.int64).reshape(-1)
    G, N, T = policy.shape
    nact = [int(a) for a in tabs["n_actions"]]
    stride = [int(np.prod(nact[i + 1:])) for i in range(N)]
    d, K, L = int(deviator), int(steps), int(dev_len)
    H = default_horizon(nact) if horizon is None else int(horizon)
    rew, sca = np.asarray(tabs["reward"], np.float64), np.asarray(tabs["scaled"], np.float64)
    gamma = np.broadcast_to(np.asarray(gamma, np.float64), (G,))
    out = {f: np.zeros(G, np.int32) for f in ("mu", "lam", "mu_post", "lam_post", "ret_step", "act_dev")}
    out.update(cycle_reward=np.zeros((N, G)), cycle_action=np.zeros((N, G)), gain=np.zeros(G),
               reward_rows=np.zeros((K, N, G)), action_rows=np.zeros((K, N, G)), horizon=H)
    for g in range(G):
        if not 0 <= start[g] < T:
            out["mu"][g], out["ret_step"][g], out["act_dev"][g] = -1, -1, -1
            continue
        F = greedy_map(tabs, policy[g])
        mu, lam, s = cycle(F, start[g], H)
        out["mu"][g], out["lam"][g] = mu, lam
        if lam > 0:
            r, a, x = np.zeros(N), np.zeros(N), s
            for _ in range(lam):
                x = int(F[x])
                r, a = r + rew[:, x], a + sca[:, x]
            out["cycle_reward"][:, g], out["cycle_action"][:, g] = r / float(lam), a / float(lam)
        y = z = s
        gain, w = np.float64(0.0), np.float64(1.0)
        for tau in range(K):
            if tau < L:
                u = int(F[y])
                ub = u - (u // stride[d] % nact[d]) * stride[d]         # the others greedy, 0 in place d
                ad = int(action)
                if ad < 0:
                    ad = int(np.argmax(rew[d, ub + np.arange(nact[d]) * stride[d]]))     # the first maximum
                if tau == 0:
                    out["act_dev"][g] = ad
                y = ub + ad * stride[d]
            else:
                y = int(F[y])
            out["reward_rows"][tau, :, g], out["action_rows"][tau, :, g] = rew[:, y], sca[:, y]
            z = int(F[z])
            gain = gain + w * (rew[d, y] - rew[d, z])
            w = w * gamma[g]
            if tau + 1 == L:
                yL = y
        out["gain"][g] = gain
        mp, lp, sp = cycle(F, yL, H)
        out["mu_post"][g], out["lam_post"][g] = mp, lp
        ret = -1
        if lam > 0 and lp > 0:
            x = sp
            for _ in range(lp):
                if x == s:
                    ret = L + mp
                    break
                x = int(F[x])
        out["ret_step"][g] = ret
    return out
