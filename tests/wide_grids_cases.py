"""The games of the wide-grid tests: QTable agents of more than 64 actions, where the action count is the width of
integer fields (the random choice of a step, the replay memory's action, the staged policies of the analyses) and not
only a loop bound.  tests/test_wide_grids_host.py runs them on the CPU oracle and asserts what each must contain;
tests/test_gpu_wide_grids.py holds the device against the same oracle runs.

Small everywhere but in the width: G <= 67 with a ragged tail (no multiple of 64), T <= 20, E <= 6, 10-50 states,
epsilon 0.5, min_memory such that every case trains.  Agents of one game differ in width, so table_off matters, and sit in
even and odd slots, so both halves of a Philox draw (x.x / x.y for even agents, x.z / x.w for odd ones) carry a wide
choice."""
import functools

import numpy as np

from oracle import oracle as O


def agent(actions, states=20, gamma=0.95, lo=0.1, hi=0.4, min_memory=None, capacity=500, **kw):
    return dict(name="QTable", gamma=gamma, actions=actions, states=states, alpha=0.1, eps_end=0.001, epsilon=0.5,
                eps_step=0.999, action_range=[lo, hi], min_memory=min_memory, capacity=capacity, **kw)


def game(agents, T, noise_prob=0.0):
    agents = [dict(a) for a in agents]
    for a in agents:
        if a["min_memory"] is None:
            a["min_memory"] = T                    # trains after every episode
    return {"agents": agents,
            "environment": dict(name="NoisyPriceState", noise_prob=noise_prob, a=10, b=1, nplayers=len(agents), max_steps=T)}


# name -> (config, G, E, seed, game_offset)
CASES = {
    # the first width past the LDS kernels' limit
    "65x65": (game([agent(65, states=10), agent(65, states=10, gamma=0.9)], T=12), 37, 4, 11, 0),
    # the widest grids whose choices a signed byte holds
    "127x128": (game([agent(127, states=17, gamma=0.9), agent(128, states=30, lo=0.05, hi=0.3)], T=13), 41, 4, 12, 5),
    # one wide agent in the even slot, a narrow one behind it
    "129x21": (game([agent(129, states=25), agent(21, states=50, gamma=0.9, min_memory=43, capacity=45)], T=20), 67, 6, 13, 0),
    # the narrow one first: the wide agent draws from x.z / x.w and its table does not start at 0
    "21x129": (game([agent(21, states=50), agent(129, states=25, gamma=0.35, min_memory=23, capacity=30)], T=20), 67, 6, 14, 1000),
    # around an unsigned byte
    "255x256": (game([agent(255, states=12, gamma=0.9), agent(256, states=12)], T=12), 67, 5, 15, 0),
    "257x1000x3": (game([agent(257, states=10), agent(1000, states=11, gamma=0.9, lo=0.0, hi=0.3), agent(3, states=40, gamma=0.35)],
                        T=20), 67, 6, 16, 7),
    # four agents, the wide one in the second Philox draw of a step
    "21x8x1000x33": (game([agent(21), agent(8, states=10, gamma=0.9), agent(1000, states=13, gamma=0.35, hi=0.2),
                           agent(33, states=50, min_memory=21, capacity=25)], T=10), 67, 6, 17, 0),
    # the env's own draws next to wide choices
    "noise-129x257": (game([agent(129, states=20, gamma=0.9), agent(257, states=15)], T=20, noise_prob=0.3), 67, 6, 18, 3),
    # tall instead of wide: the largest row index the 16-bit replay memory of the generic kernel has to hold
    "tall-32000": (game([agent(2, states=32000), agent(2, states=32000, gamma=0.9)], T=15), 5, 4, 19, 0),
}
DTYPES = ("float32", "float64")


def n_actions(name):
    return [int(a["actions"]) for a in CASES[name][0]["agents"]]


def eps_schedule(cfg, eps0, E):
    """[E, N]: epsilon during episode e (it decays after every episode's train_net, agents.py:78)."""
    L = O.lib()
    out = np.zeros((E, cfg.n_agents))
    eps = [float(x) for x in eps0[:cfg.n_agents]]
    for e in range(E):
        out[e] = eps
        eps = [L.oracle_eps_decay(eps[i], cfg.eps_end[i], cfg.eps_step[i]) for i in range(cfg.n_agents)]
    return out


def step_draws(n_act, G, seed, game_offset, episode, step, noise=False):
    """One lockstep step's draws from oracle.philox, as thrl_op_draws returns them: (u [N, G] float64, word [N, G] uint32
    -- the word behind the choice --, choice [N, G] int64 = (word * A) >> 32 in 64-bit arithmetic, noise words [2, G] or
    None).  Counter layout: DESIGN.md "RNG"."""
    N = len(n_act)
    u = np.zeros((N, G)); w = np.zeros((N, G), np.uint32); nz = np.zeros((2, G), np.uint32) if noise else None
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    for g in range(G):
        gid = game_offset + g
        hi = (gid >> 32) & 0xFFFFFF
        for pair in range((N + 1) // 2):
            x = O.philox([step & 0xFFFFFFFF, episode & 0xFFFFFFFF, gid & 0xFFFFFFFF, hi | (pair << 24)], key)
            for h in range(2):
                i = 2 * pair + h
                if i < N:
                    u[i, g] = x[2 * h] * 2.0 ** -32
                    w[i, g] = x[2 * h + 1]
        if noise:
            x = O.philox([step & 0xFFFFFFFF, episode & 0xFFFFFFFF, gid & 0xFFFFFFFF, hi | (0x40 << 24)], key)
            nz[0, g], nz[1, g] = x[0], x[1]
    choice = (w.astype(np.uint64) * np.asarray(n_act, np.uint64)[:, None]) >> np.uint64(32)
    return u, w, choice.astype(np.int64), nz


@functools.lru_cache(maxsize=None)
def run_draws(name):
    """(u, choice) [E, T, N, G] of the whole run of a case."""
    config, G, E, seed, off = CASES[name]
    T = int(config["environment"]["max_steps"])
    A = n_actions(name)
    u = np.zeros((E, T, len(A), G)); ch = np.zeros((E, T, len(A), G), np.int64)
    for e in range(E):
        for t in range(T):
            u[e, t], _, ch[e, t], _ = step_draws(A, G, seed, off, e, t)
    u.setflags(write=False); ch.setflags(write=False)
    return u, ch


@functools.lru_cache(maxsize=None)
def oracle_run(name, dtype):
    """The oracle's run of a case from its own initial tables: dict(q0, s0, q, counter, state, eps, trace_actions,
    trace_price, mem_count).  Computed once per module run; the arrays are read-only."""
    config, G, E, seed, off = CASES[name]
    cfg, eps = O.cfg_from_config(config, G, 1 if dtype == "float64" else 0)
    q0, _, s0 = O.init(cfg, seed, off)
    q, s, c = q0.copy(), s0.copy(), np.zeros(q0.shape, np.int32)
    mem = O.Memory(cfg)
    out = O.episodes(cfg, q, c, s, eps, mem, E, seed=seed, game_offset=off, trace=True)
    res = dict(q0=q0, s0=s0, q=q, counter=c, state=s, eps=eps.copy(), trace_actions=out["trace_actions"],
               trace_price=out["trace_price"], mem_count=mem.count.copy(), game_reward_log=out["game_reward_log"],
               game_action_log=out["game_action_log"])
    for v in res.values():
        v.setflags(write=False)
    return res


def trained_steps(config, E):
    """Per agent, the (episode, step) pairs whose transitions train_net replayed during E episodes, in replay order:
    the deque bookkeeping of buffers.py / agents.py:59-78, which is the same for every game."""
    T = int(config["environment"]["max_steps"])
    out = []
    for a in config["agents"]:
        cap, need = int(a["capacity"]), int(a["min_memory"])
        buf, got = [], []
        for e in range(E):
            for t in range(T):
                buf.append((e, t))
            buf = buf[-cap:] if cap > 0 else []
            if len(buf) >= need:
                got.append(list(buf))
                buf = []
        out.append(got)
    return out


def planted_tables(config, G, dtype, seed=0):
    """[G, stride] random tables whose rows have a planted maximum where a narrow policy field loses it: in turn at the
    last action, at 255, at 256 (where the agent has them) and at a low index.  A policy truncated to 8 bits, or read with
    the wrong width, then plays another action."""
    cfg, _ = O.cfg_from_config(config, G, 1 if dtype == "float64" else 0)
    rs = np.random.RandomState(seed)
    q = rs.normal(0.0, 1.0, (G, O.table_stride(cfg))).astype(np.float64 if dtype == "float64" else np.float32)
    for i, a in enumerate(config["agents"]):
        A, rows, off = int(a["actions"]), int(a["states"]) + 1, O.table_offset(cfg, i)
        spots = [c for c in (A - 1, 255, 256, 3) if c < A]
        tab = q[:, off:off + rows * A].reshape(G, rows, A)
        pick = rs.randint(0, len(spots), (G, rows))
        for k, c in enumerate(spots):
            g, r = np.nonzero(pick == k)
            tab[g, r, c] = 10.0 + rs.uniform(0, 1, len(g))
        q[:, off:off + rows * A] = tab.reshape(G, rows * A)
    return q
