"""The limit table of the episode kernels' eligibility plans (thrl_api.hip: plan_wave, plan_tuple, plan_ptuple;
thrl_mixed.hip: plan_mixed), shared by test_limits_host.py (CPU) and test_gpu_limits.py (GPU).

Every NO(...) reason of the four plans is listed in REASONS with either the ids of an accepted / refused pair of
CASES, a note why only one side exists, or "unreachable" (proved by enumeration in test_limits_host.py).  A case is a
reference-schema config at the last value a plan accepts or the first one it refuses; `expect` names the quantity that
sits on the limit, restated here in numpy / plain Python from the plans' formulas (not read from the library), so
that a moved limit and a drifted config both show up on the host.

Unless the limit is about them: a=10, b=1, max_state=10.  G and E stay tiny; E is one training cycle (two launches
where the issue asks for them), E2 one more cycle for the second run() call."""
import numpy as np

LDS_PER_CU = 160 * 1024            # MI355X; the plans read it from the device

Q = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001, epsilon=0.5, eps_step=0.9995,
         action_range=[0.2, 0.4])
QTABLE_DEFAULTS = dict(capacity=500, min_memory=100, max_state=10)
NN_DEFAULTS = dict(capacity=50000, min_memory=1000)


def qa(**kw):
    return dict(Q, **kw)


def game(agents, T, noise=0.0):
    return {"agents": [dict(a) for a in agents],
            "environment": dict(name="NoisyPriceState", noise_prob=noise, a=10, b=1, nplayers=len(agents), max_steps=T)}


# ---------------------------------------------------------------------------------------------------------------
# restatement of the plans' arithmetic


def _kind(a):
    return a.get("name", "QTable")


def _quantities(config):
    """Per agent (a/b) * scale_i(k), k = 0..A_i-1: QTable.scale divides by A - 1, Reinforce.scale by A."""
    env = config["environment"]
    ratio = float(env["a"]) / float(env["b"])
    out = []
    for ag in config["agents"]:
        A = int(ag["actions"])
        lo, hi = float(ag["action_range"][0]), float(ag["action_range"][1])
        den = float(A) - 1.0 if _kind(ag) == "QTable" else float(A)
        out.append(ratio * (np.arange(A, dtype=np.float64) / den * (hi - lo) + lo))
    return out


def prices(config, intercept=None):
    """float64 price of every action tuple (first agent = slowest digit), summed in agent order as the plans do."""
    env = config["environment"]
    a = float(env["a"]) if intercept is None else float(intercept)
    Qs = np.zeros((1,), np.float64)
    for q in _quantities(config):
        Qs = (Qs[:, None] + q[None, :]).reshape(-1)
    p = a - float(env["b"]) * Qs
    return np.where(p > 0.0, p, 0.0)


def encode64(p, max_state, states):
    return np.rint(p / float(max_state) * float(states)).astype(np.int64)


def encode32(p, max_state, states):
    x = p.astype(np.float32) / np.float32(max_state) * np.float32(states)
    return np.rint(x).astype(np.int64)


def window(config, agent):
    """(row_lo, win_rows, inside) of a QTable agent: both encodes of every tuple's price, with noise also at 0.7 a."""
    env, ag = config["environment"], config["agents"][agent]
    ms, S = ag.get("max_state", 10), int(ag["states"])
    ps = [prices(config)]
    if float(env.get("noise_prob", 0)) > 0.0:
        ps.append(prices(config, float(env["a"]) * 0.7))
    rows = np.concatenate([f(p, ms, S) for p in ps for f in (encode64, encode32)])
    lo, hi = int(rows.min()), int(rows.max())
    return lo, hi - lo + 1, bool(lo >= 0 and hi <= S)


def cycle(config, agent=0):
    """(epk, keep) of the wave kernel's training cycle: trains every epk = ceil(min_memory / T)-th episode on the last
    keep = min(epk * T, capacity) transitions; (0, 0) = never trains (capacity < min_memory)."""
    ag = dict(QTABLE_DEFAULTS, **config["agents"][agent])
    T, cap, mm = int(config["environment"]["max_steps"]), int(ag["capacity"]), max(int(ag["min_memory"]), 1)
    if cap < mm or cap <= 0:
        return 0, 0
    epk = -(-mm // T)
    return epk, min(epk * T, cap)


def n_tuples(config):
    return int(np.prod([int(a["actions"]) for a in config["agents"]], dtype=np.int64))


def field_bits(A):
    bits = 0
    while (1 << bits) < A:
        bits += 1
    return bits


def action_word_bits(actions):
    """Width of the tuple kernel's action word: one field of ceil(log2 A_i) bits per agent, from bit 1."""
    return 1 + sum(field_bits(int(A)) for A in actions)


def wave_game_lds_bytes(config, dtype):
    lo, W, _ = window(config, 0)
    A = int(config["agents"][0]["actions"])
    n = 2 * (W + 2) * A * (8 if dtype == "float64" else 4)
    if dtype == "float32" and not float(config["environment"].get("noise_prob", 0)) > 0.0:
        n += 256
    return n


def _up(x, a):
    return (x + a - 1) // a * a


def tuple_lds_bytes(config, dtype):
    """(lut_lds_bytes, game_lds_bytes) of plan_tuple."""
    esz = 8 if dtype == "float64" else 4
    N, tuples = len(config["agents"]), n_tuples(config)
    elems = am = 0
    for i, ag in enumerate(config["agents"]):
        W = window(config, i)[1]
        cells = (W + 2) * int(ag["actions"])
        elems += (cells + 3) & ~3
        am += (W + 2 + 3) & ~3
    am_off = _up(elems * esz, 16)
    g_off = _up(am_off + am, 16)
    game = _up(g_off + 2 * (tuples + 1), 16)
    lut = _up(tuples * 8, 16) + N * 64 * 8 * 2
    return lut, game


def waves_per_block_that_fit(lut, game):
    return max([w for w in range(1, 17) if lut + w * game <= LDS_PER_CU] or [0])


def distinct_prices(config):
    """Distinct float32 prices over the action pairs (the policy-tuple kernel's price ids)."""
    return int(np.unique(prices(config).astype(np.float32).view(np.uint32)).size)


def ptuple_lds_bytes(config, dtype):
    """(lut_lds_bytes, game_lds_bytes, cdf_bytes) of plan_ptuple for a two-agent game with a neural agent."""
    esz = 8 if dtype == "float64" else 4
    tuples, npid = n_tuples(config), distinct_prices(config)
    kinds = [_kind(a) for a in config["agents"]]
    amax = max(int(a["actions"]) for a, k in zip(config["agents"], kinds) if k != "QTable")
    apad = 24 if amax <= 24 else 32
    off = cdf = 0
    if "QTable" in kinds:
        qi = kinds.index("QTable")
        W = window(config, qi)[1]
        cells = (W + 2) * int(config["agents"][qi]["actions"])
        off = _up(cells * esz, 16)
        off = _up(off + W + 2, 16)
        off = _up(off + tuples + 1, 16)
        off = _up(off + 4 * ((cells + 1) // 2), 16)
    else:
        cdf = 2 * (npid + 1) * apad * 4
        off = _up(off + cdf, 16)
    off += 64 * 4 * 8
    game = _up(off, 16)
    qrows = _up(tuples * 2, 16)
    xf = _up(qrows + tuples * 2, 16)
    aq = _up(xf + npid * 4, 16)
    return aq + 2 * 128 * 8, game, cdf


def mixed_lds_bytes(config, dtype):
    """plan_mixed's LDS bytes of one all-QTable game (no CAC network, no policy memo)."""
    esz = 8 if dtype == "float64" else 4
    N = len(config["agents"])
    off = sum(((int(a["states"]) + 1) * int(a["actions"]) + 3) & ~3 for a in config["agents"])
    n = _up(N * 64 * 8 + off * esz, 16)
    return _up(n + 16 * 8 + 16 * N * 12, 16)


def ring_len(agent, T):
    """MixedGameBatch's ring of one agent: at most min_memory + T entries before a train call empties it."""
    d = dict(QTABLE_DEFAULTS if _kind(agent) == "QTable" else NN_DEFAULTS, **agent)
    cap, mm = int(d["capacity"]), int(d["min_memory"])
    return min(cap, mm + T) if cap >= mm else cap


def measure(case):
    """Every quantity a case's `expect` may name."""
    c, dt = case["config"], case["dtypes"][0]
    T = int(c["environment"]["max_steps"])
    kinds = [_kind(a) for a in c["agents"]]
    m = dict(T=T, n_agents=len(kinds), tuples=n_tuples(c), max_actions=max(int(a["actions"]) for a in c["agents"]),
             word_bits=action_word_bits([a["actions"] for a in c["agents"]]))
    qs = [i for i, k in enumerate(kinds) if k == "QTable"]
    if qs:
        wins = [window(c, i) for i in qs]
        m.update(win_rows=max(w[1] for w in wins), inside=all(w[2] for w in wins),
                 q_actions=max(int(c["agents"][i]["actions"]) for i in qs))
        epk, keep = cycle(c, qs[0])
        m.update(epk=epk, keep=keep, transitions=epk * T, replay_from=epk * T - keep, E=case["E"])
        d = dict(QTABLE_DEFAULTS, **c["agents"][qs[0]])
        m.update(once_per_episode=all(dict(QTABLE_DEFAULTS, **c["agents"][i])["min_memory"] <= T
                                      <= dict(QTABLE_DEFAULTS, **c["agents"][i])["capacity"] for i in qs),
                 q_ring=ring_len(c["agents"][qs[0]], T), q_min_memory=int(d["min_memory"]))
    if case["plan"] == "wave":
        m["wave_game_lds"] = wave_game_lds_bytes(c, dt)
    if case["plan"] == "tuple" and m.get("inside") and m["tuples"] <= 8192 and len(kinds) <= 4:
        lut, gm = tuple_lds_bytes(c, dt)
        m.update(tuple_lds_one_wave=lut + gm, tuple_waves=waves_per_block_that_fit(lut, gm))
    if case["plan"] == "ptuple":
        nn = [i for i, k in enumerate(kinds) if k != "QTable"]
        m.update(nn_actions=max(int(c["agents"][i]["actions"]) for i in nn), prices=distinct_prices(c),
                 nn_ring=min(ring_len(c["agents"][i], T) for i in nn))
        lut, gm, cdf = ptuple_lds_bytes(c, dt)
        m.update(ptuple_lds_one_wave=lut + gm, cdf_bytes=cdf)
    if case["plan"] == "mixed":
        m["mixed_lds"] = mixed_lds_bytes(c, dt)
    return m


# ---------------------------------------------------------------------------------------------------------------
# the cases

BOTH = ("float32", "float64")
CASES = []


def case(id, plan, side, config, expect, reason=None, falls_to=None, G=5, E=2, E2=None, dtypes=BOTH, kind=None):
    """side: "accept" (the plan's kernel runs it) or "refuse" (forcing raises `reason`, auto runs `falls_to`;
    falls_to=None: auto is not run).  kind: the neural agent class of a policy-tuple case."""
    CASES.append(dict(id=id, plan=plan, side=side, config=config, expect=expect, reason=reason, falls_to=falls_to,
                      G=G, E=E, E2=E if E2 is None else E2, dtypes=tuple(dtypes), kind=kind))


def two(agent, T, noise=0.0):
    return game([agent, agent], T, noise)


# ---- wave kernel (two identical QTable grids)
WIDE = qa(states=125, action_range=[0, 0.5])                       # prices 10 .. 0: every row of the table
case("wave-rows-126", "wave", "accept", two(WIDE, 100), dict(win_rows=126, epk=1))
case("wave-rows-127", "wave", "refuse", two(dict(WIDE, states=126), 100), dict(win_rows=127),
     reason="reachable row window > 126 rows", falls_to="tuple")
case("wave-rows-126-noise", "wave", "accept", two(WIDE, 100, 0.2), dict(win_rows=126))
case("wave-rows-127-noise", "wave", "refuse", two(dict(WIDE, states=126), 100, 0.2), dict(win_rows=127),
     reason="reachable row window > 126 rows", falls_to="tuple")
# the largest LDS footprint of one game: 2 x 128 rows x 32 actions x 8 B
case("wave-rows-126-A32-f64", "wave", "accept", two(dict(WIDE, actions=32), 100),
     dict(win_rows=126, max_actions=32, wave_game_lds=65536), dtypes=("float64",))
case("wave-A32", "wave", "accept", two(qa(actions=32), 100), dict(max_actions=32))
case("wave-A33", "wave", "refuse", two(qa(actions=33), 100), dict(max_actions=33), reason="actions > 32", falls_to="tuple")
case("wave-256-transitions", "wave", "accept", two(qa(min_memory=256), 64), dict(epk=4, transitions=256, keep=256), E=4)
case("wave-320-transitions", "wave", "refuse", two(qa(min_memory=257), 64), dict(epk=5, transitions=320),
     reason="more than 256 transitions per training cycle", falls_to="generic", E=5)
# the same limit one transition apart: a single episode of 256 / 257 steps (the tuple kernel stops at 256 steps too)
case("wave-T256", "wave", "accept", two(qa(), 256), dict(epk=1, transitions=256, keep=256), G=3, E=2, E2=1)
case("wave-T257", "wave", "refuse", two(qa(), 257), dict(epk=1, transitions=257),
     reason="more than 256 transitions per training cycle", falls_to="generic", G=3, E=2, E2=1)
case("wave-epk32-T7", "wave", "accept", two(qa(min_memory=224), 7), dict(epk=32, transitions=224), G=3, E=64, E2=32)
case("wave-epk32-T1", "wave", "accept", two(qa(min_memory=32), 1), dict(epk=32, transitions=32), G=3, E=64, E2=32)
case("wave-epk33-T7", "wave", "refuse", two(qa(min_memory=225), 7), dict(epk=33, transitions=231),
     reason="more than 32 episodes per training cycle", falls_to="generic", G=3, E=33)
# keep = min(epk * T, capacity): the whole cycle is replayed / its first transition has left the deque
case("wave-keep-all", "wave", "accept", two(qa(min_memory=25, capacity=30), 10), dict(epk=3, keep=30, replay_from=0), E=3)
case("wave-keep-all-but-one", "wave", "accept", two(qa(min_memory=25, capacity=29), 10), dict(epk=3, keep=29, replay_from=1), E=3)
case("wave-keep-256", "wave", "accept", two(qa(min_memory=250, capacity=256), 64), dict(epk=4, keep=256, replay_from=0), E=4)
case("wave-keep-255", "wave", "accept", two(qa(min_memory=250, capacity=255), 64), dict(epk=4, keep=255, replay_from=1), E=4)
# capacity = min_memory trains on exactly min_memory transitions; one less never trains (both run on the wave kernel)
case("wave-trains", "wave", "accept", two(qa(min_memory=25, capacity=25), 10), dict(epk=3, keep=25, replay_from=5), E=3)
case("wave-never-trains", "wave", "accept", two(qa(min_memory=25, capacity=24), 10), dict(epk=0, keep=0), E=3)
# the register variant of the float32 kernel switches at T * epk > 128 (both sides run)
case("wave-cycle-128", "wave", "accept", two(qa(min_memory=128), 64), dict(epk=2, transitions=128), E=2)
case("wave-cycle-129", "wave", "accept", two(qa(min_memory=129), 43), dict(epk=3, transitions=129), E=3)
case("wave-whole-cycles", "wave", "accept", two(qa(min_memory=25), 10), dict(epk=3, E=3), E=3)
case("wave-partial-cycle", "wave", "refuse", two(qa(min_memory=25), 10), dict(epk=3, E=4),
     reason="episodes of this call are not a multiple of the training cycle", falls_to="generic", E=4)
# the top price a = 10 encodes to rint(10 / max_state * 100): row 100 at 9.96, row 101 (outside) at 9.95.  The reference
# raises IndexError there and the generic kernel does not clamp, so the refused side is only forced, never run.
EDGE = qa(action_range=[0, 0.5])
case("wave-top-row-inside", "wave", "accept", two(dict(EDGE, max_state=9.96), 100), dict(inside=True, win_rows=101))
case("wave-top-row-outside", "wave", "refuse", two(dict(EDGE, max_state=9.95), 100), dict(inside=False),
     reason="price outside the table on the action grid", falls_to=None)

# ---- tuple kernel (1-4 QTable agents, individual grids, every agent trains once per episode)
TQ = qa(min_memory=10)
B64 = [dict(TQ, actions=64, states=40, action_range=[0.0, 0.3]), dict(TQ, actions=64, states=60, action_range=[0.1, 0.4])]
case("tuple-4096", "tuple", "accept", game(B64, 20), dict(tuples=4096, max_actions=64))
case("tuple-8192", "tuple", "refuse", game(B64 + [dict(TQ, actions=2, states=16, action_range=[0.0, 0.1])], 20),
     dict(tuples=8192), reason="more than 4,096 action tuples", falls_to="generic")
FOUR8 = [dict(TQ, actions=8, states=s, action_range=[0.0, 0.2]) for s in (20, 30, 40, 50)]
case("tuple-4096-four-agents", "tuple", "accept", game(FOUR8, 20), dict(tuples=4096, n_agents=4, word_bits=13))
SMALL = dict(TQ, actions=3, states=16, action_range=[0.0, 0.25])
case("tuple-A64", "tuple", "accept", game([dict(TQ, actions=64, states=50, action_range=[0.0, 0.3]), SMALL], 20),
     dict(max_actions=64))
case("tuple-A65", "tuple", "refuse", game([dict(TQ, actions=65, states=50, action_range=[0.0, 0.3]), SMALL], 20),
     dict(max_actions=65), reason="more than 64 actions", falls_to="generic")
W16 = [dict(TQ, actions=A, states=s, action_range=[0.0, 0.2]) for A, s in ((9, 20), (9, 30), (9, 40), (5, 50))]
case("tuple-word-16-bits", "tuple", "accept", game(W16, 20), dict(word_bits=16, tuples=3645))
TWIDE = dict(TQ, states=253, action_range=[0, 0.5])
case("tuple-rows-254", "tuple", "accept", two(TWIDE, 20), dict(win_rows=254))
case("tuple-rows-255", "tuple", "refuse", two(dict(TWIDE, states=254), 20), dict(win_rows=255),
     reason="reachable row window > 254 rows", falls_to="generic")
LONG = [dict(TQ, actions=4, states=16, action_range=[0.0, 0.25], capacity=600),
        dict(TQ, actions=5, states=40, action_range=[0.05, 0.2], capacity=600)]
case("tuple-T256", "tuple", "accept", game(LONG, 256), dict(T=256), G=3, E=2, E2=1)
case("tuple-T257", "tuple", "refuse", game(LONG, 257), dict(T=257), reason="more than 256 steps per episode",
     falls_to="generic", G=3, E=2, E2=1)
B64L = [dict(a, capacity=600) for a in B64]
case("tuple-T256-4096", "tuple", "accept", game(B64L, 256), dict(T=256, tuples=4096), G=3, E=2, E2=1)
case("tuple-T257-4096", "tuple", "refuse", game(B64L, 257), dict(T=257, tuples=4096),
     reason="more than 256 steps per episode", falls_to="generic", G=3, E=2, E2=1)
RB = [dict(TQ, actions=7, states=30, action_range=[0.1, 0.5]), dict(TQ, actions=4, states=16, action_range=[0.0, 0.25])]


def _rb(**kw):
    return game([dict(a, **kw) for a in RB], 20)


REPLAY = "replay buffer does not fill / train once per episode"
case("tuple-buffer-exact", "tuple", "accept", _rb(min_memory=20, capacity=20), dict(once_per_episode=True))
case("tuple-buffer-short", "tuple", "refuse", _rb(min_memory=20, capacity=19), dict(once_per_episode=False),
     reason=REPLAY, falls_to="generic")
case("tuple-buffer-late", "tuple", "refuse", _rb(min_memory=21, capacity=500), dict(once_per_episode=False),
     reason=REPLAY, falls_to="generic")
# float64, 64 x 64 actions: LDS holds one wave's game up to states = 114 (116 rows + 2 per agent; found from
# lut_lds_bytes + game_lds_bytes <= 160 KiB: 34,816 + 128,256 = 163,072 B; states = 115 needs 164,096 B)
LDS64 = dict(TQ, actions=64, states=114, action_range=[0, 0.5])
case("tuple-lds-one-wave", "tuple", "accept", two(LDS64, 20), dict(tuple_waves=1, tuple_lds_one_wave=163072),
     dtypes=("float64",), G=3)
case("tuple-lds-none", "tuple", "refuse", two(dict(LDS64, states=115), 20), dict(tuple_waves=0, tuple_lds_one_wave=164096),
     reason="tables of one game do not fit LDS", falls_to="generic", dtypes=("float64",), G=3)
FOUR4 = [dict(TQ, actions=4, states=s, action_range=[0.0, 0.2]) for s in (20, 30, 40, 50)]
case("tuple-four-agents", "tuple", "accept", game(FOUR4, 20), dict(n_agents=4))
case("tuple-five-agents", "tuple", "refuse", game(FOUR4 + [dict(TQ, actions=4, states=16, action_range=[0.0, 0.2])], 20),
     dict(n_agents=5), reason="more than 4 agents", falls_to="generic")
TE = [dict(TQ, actions=7, states=30, action_range=[0.0, 0.5]), dict(TQ, actions=5, action_range=[0.0, 0.5])]
case("tuple-top-row-inside", "tuple", "accept", game([TE[0], dict(TE[1], max_state=9.96)], 20), dict(inside=True))
case("tuple-top-row-outside", "tuple", "refuse", game([TE[0], dict(TE[1], max_state=9.95)], 20), dict(inside=False),
     reason="price outside a table on the action grid", falls_to=None)

# ---- policy-tuple kernel (two agents, at least one Reinforce / ActorCritic); the reference is the operator loop.
# `kind` replaces the name of every agent called "NN".  A refused config runs on the general mixed kernel
# (episode_kernel "wave") unless that one refuses it too ("unfused": the operator loop; "error": the constructor).
PT = 10


def pq(**kw):
    return qa(**dict(dict(min_memory=PT, capacity=500), **kw))


def nn(**kw):
    return dict(dict(name="NN", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4], min_memory=PT, entropy=0.01), **kw)


def pcase(id, side, agents, expect, T=PT, falls_to=None, reason=None, dtypes=BOTH, G=3, E=3, E2=2, kinds=("Reinforce", "ActorCritic")):
    for k in kinds:
        ags = [dict(a, name=k) if a.get("name") == "NN" else dict(a) for a in agents]
        case("%s-%s" % (id, k), "ptuple", side, game(ags, T), expect, reason=reason, falls_to=falls_to, G=G, E=E, E2=E2,
             dtypes=dtypes, kind=k)


pcase("ptuple-nn-A32", "accept", [pq(), nn(actions=32)], dict(nn_actions=32))
pcase("ptuple-nn-A33", "refuse", [pq(), nn(actions=33)], dict(nn_actions=33), falls_to="error", reason="2 <= actions <= 32")
pcase("ptuple-q-A64", "accept", [pq(actions=64), nn()], dict(q_actions=64))
pcase("ptuple-q-A65", "refuse", [pq(actions=65), nn()], dict(q_actions=65), falls_to="unfused",
      reason="QTable agent with more than 64 actions")
pcase("ptuple-T256", "accept", [pq(min_memory=256), nn(min_memory=256)], dict(T=256), T=256, G=2, E=2, E2=1)
pcase("ptuple-T257", "refuse", [pq(min_memory=257), nn(min_memory=257)], dict(T=257), T=257, falls_to="wave", G=2, E=2, E2=1)
# 64 x 32 action pairs is the most a QTable and a neural agent can have, and with the neural step = 1/32 of the QTable's every
# pair has its own price: 2,048 of each, the limits themselves ("more than" either is unreachable, test_limits_host.py)
pcase("ptuple-2048-pairs-2048-prices", "accept",
      [pq(actions=64, action_range=[0, 0.7875]), nn(actions=32, action_range=[0, 0.0125])], dict(tuples=2048, prices=2048))
PWIDE = pq(states=253, action_range=[0, 0.6])
pcase("ptuple-rows-254", "accept", [PWIDE, nn(action_range=[0, 0.5])], dict(win_rows=254))
pcase("ptuple-rows-255", "refuse", [dict(PWIDE, states=254), nn(action_range=[0, 0.5])], dict(win_rows=255), falls_to="wave")
pcase("ptuple-nn-ring-one-episode", "accept", [pq(), nn(capacity=PT)], dict(nn_ring=PT))
pcase("ptuple-nn-ring-one-short", "refuse", [pq(), nn(capacity=PT - 1)], dict(nn_ring=PT - 1), falls_to="wave")
pcase("ptuple-q-ring-one-episode", "accept", [pq(capacity=PT), nn()], dict(q_ring=PT, q_min_memory=PT))
pcase("ptuple-q-ring-one-short", "refuse", [pq(capacity=PT - 1), nn()], dict(q_ring=PT - 1), falls_to="wave")
pcase("ptuple-q-trains-late", "refuse", [pq(min_memory=PT + 1), nn()], dict(q_min_memory=PT + 1), falls_to="wave")
# two neural agents keep both CDF tables in LDS: 2 x (prices + 1) x 32 x 4 B <= 24 KiB, i.e. at most 95 prices.  32 x 3 actions
# with the second step 15.5 x the first: (31, 0) and (0, 2) share a price, 95 in all; at 15.75 x none do, 96
NN32 = dict(name="Reinforce", gamma=0.995, actions=32, states=1, action_range=[0, 0.32], min_memory=PT, entropy=0.01)
pcase("ptuple-cdf-24KiB", "accept", [NN32, nn(actions=3, action_range=[0, 0.465])], dict(prices=95, cdf_bytes=24576),
      kinds=("ActorCritic",))
pcase("ptuple-cdf-over", "refuse", [NN32, nn(actions=3, action_range=[0, 0.4725])], dict(prices=96, cdf_bytes=24832),
      falls_to="wave", kinds=("ActorCritic",))
# float64 QTable of 64 actions against 21: the largest window that fits one wave's LDS (found from lut_lds_bytes +
# game_lds_bytes <= 160 KiB: 8,272 + 155,328 = 163,600 B) is 235 rows = states 234 on [0, 0.6], states 235 needs 164,240 B; the general kernel cannot hold such a table either
PLDS = pq(actions=64, states=234, action_range=[0, 0.6])
pcase("ptuple-lds-fits", "accept", [PLDS, nn(action_range=[0, 0.5])], dict(ptuple_lds_one_wave=163600), dtypes=("float64",), G=2)
pcase("ptuple-lds-over", "refuse", [dict(PLDS, states=235), nn(action_range=[0, 0.5])], dict(ptuple_lds_one_wave=164240),
      falls_to="unfused", reason="exceed 64 KiB of LDS", dtypes=("float64",), G=2)

# ---- general mixed kernel: one game's tables at 64 KiB of LDS (all-QTable games: the reference is the CPU oracle)
MQ = qa(actions=20, min_memory=10)
case("mixed-64KiB-f32", "mixed", "accept", game([dict(MQ, states=399), dict(MQ, states=399)], 10), dict(mixed_lds=65536),
     dtypes=("float32",), G=3, E=3)
case("mixed-over-64KiB-f32", "mixed", "refuse", game([dict(MQ, states=399), dict(MQ, states=400)], 10), dict(mixed_lds=65616),
     reason="exceed 64 KiB of LDS", falls_to="unfused", dtypes=("float32",), G=3, E=3)
case("mixed-64KiB-f64", "mixed", "accept", game([dict(MQ, states=199), dict(MQ, states=199)], 10), dict(mixed_lds=65536),
     dtypes=("float64",), G=3, E=3)
case("mixed-over-64KiB-f64", "mixed", "refuse", game([dict(MQ, states=199), dict(MQ, states=200)], 10), dict(mixed_lds=65696),
     reason="exceed 64 KiB of LDS", falls_to="unfused", dtypes=("float64",), G=3, E=3)
case("mixed-q-A64", "mixed", "accept", game([dict(MQ, actions=64, states=50), dict(MQ, states=50)], 10), dict(q_actions=64),
     G=3, E=3)
case("mixed-q-A65", "mixed", "refuse", game([dict(MQ, actions=65, states=50), dict(MQ, states=50)], 10), dict(q_actions=65),
     reason="QTable agent with more than 64 actions", falls_to="unfused", G=3, E=3)

BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)

# ---------------------------------------------------------------------------------------------------------------
# every NO(...) reason of the four plans: (plan, reason) -> ("pair", accepted id, refused id) | ("note", why only one
# side exists) | ("unreachable", why; proved in test_limits_host.py)
REASONS = {
    ("wave", "needs exactly 2 agents"): ("note", "a count, not a size: three agents are the tuple kernel's (tuple-four-agents)"),
    ("wave", "agents must share the state/action grid sizes"): ("note", "an equality, not a size: every tuple case with two agents"),
    ("wave", "actions > 32"): ("pair", "wave-A32", "wave-A33"),
    ("wave", "the agents' replay buffers fill / train on different cycles"): ("note", "an equality of the two agents' cycles, not a size (test_host_cpu.py)"),
    ("wave", "non-empty replay memory on entry"): ("note", "run state, not configuration: only the generic kernel leaves a buffer filled"),
    ("wave", "more than 256 transitions per training cycle"): ("pair", "wave-256-transitions", "wave-320-transitions"),
    ("wave", "more than 32 episodes per training cycle"): ("pair", "wave-epk32-T7", "wave-epk33-T7"),
    ("wave", "episodes of this call are not a multiple of the training cycle"): ("pair", "wave-whole-cycles", "wave-partial-cycle"),
    ("wave", "price outside the table on the action grid"): ("pair", "wave-top-row-inside", "wave-top-row-outside"),
    ("wave", "reachable row window > 126 rows"): ("pair", "wave-rows-126", "wave-rows-127"),
    ("wave", "table window does not fit LDS"): ("unreachable", "128 rows x 32 actions x 8 B x 2 agents + the LUT is under 160 KiB"),
    ("tuple", "more than 4 agents"): ("pair", "tuple-four-agents", "tuple-five-agents"),
    ("tuple", "more than 256 steps per episode"): ("pair", "tuple-T256", "tuple-T257"),
    ("tuple", "more than 64 actions"): ("pair", "tuple-A64", "tuple-A65"),
    ("tuple", "more than 4,096 action tuples"): ("pair", "tuple-4096", "tuple-8192"),
    ("tuple", "replay buffer does not fill / train once per episode"): ("pair", "tuple-buffer-exact", "tuple-buffer-short"),
    ("tuple", "non-empty replay memory on entry"): ("note", "run state, not configuration"),
    ("tuple", "price outside a table on the action grid"): ("pair", "tuple-top-row-inside", "tuple-top-row-outside"),
    ("tuple", "reachable row window > 254 rows"): ("pair", "tuple-rows-254", "tuple-rows-255"),
    ("tuple", "more than 65,535 resident table cells per agent"): ("unreachable", "at most 256 rows x 64 actions = 16,384 cells"),
    ("tuple", "visit histogram does not fit the table region"): ("unreachable", "2 B per cell against at least 4 B per cell"),
    ("tuple", "action word wider than 16 bits"): ("unreachable", "field widths sum to at most 15 under 4,096 tuples"),
    ("tuple", "LUT image too large"): ("unreachable", "24 B x 4,096 tuples + 4 KiB is under 160 KiB"),
    ("tuple", "tables of one game do not fit LDS"): ("pair", "tuple-lds-one-wave", "tuple-lds-none"),
    ("ptuple", "not a two-agent game"): ("note", "a count, not a size"),
    ("ptuple", "more than 256 steps per episode"): ("pair", "ptuple-T256-Reinforce", "ptuple-T257-Reinforce"),
    ("ptuple", "no neural agent"): ("note", "agent kinds, not a size: two QTables are the wave / tuple kernels' (mixed-64KiB-f32)"),
    ("ptuple", "QTable agent with more than 64 actions"): ("pair", "ptuple-q-A64-Reinforce", "ptuple-q-A65-Reinforce"),
    ("ptuple", "QTable replay buffer does not train once per episode"): ("pair", "ptuple-q-ring-one-episode-Reinforce", "ptuple-q-ring-one-short-Reinforce"),
    ("ptuple", "neural agent with more than 32 actions"): ("pair", "ptuple-nn-A32-Reinforce", "ptuple-nn-A33-Reinforce"),
    ("ptuple", "a neural agent's replay ring is shorter than an episode"): ("pair", "ptuple-nn-ring-one-episode-Reinforce", "ptuple-nn-ring-one-short-Reinforce"),
    ("ptuple", "continuous agent"): ("note", "an agent kind, not a size (test_gpu_fuzz.py mixes CAC agents in)"),
    ("ptuple", "noise_prob sweep without a QTable agent in the game"): ("note", "a sweep argument, not a size"),
    ("ptuple", "epsilon-schedule sweep without a per-game epsilon array (sweep_eps)"): ("note", "a sweep argument, not a size"),
    ("ptuple", "more than 4,096 action pairs"): ("unreachable", "at most 64 x 32 = 2,048 pairs pass the action checks before it (ptuple-2048-pairs-2048-prices)"),
    ("ptuple", "price outside the table on the action grid"): ("note", "the same arithmetic as the tuple kernel's (tuple-top-row-outside); the general kernel does not clamp, so not run"),
    ("ptuple", "more than 2,048 distinct prices"): ("unreachable", "no more prices than pairs, at most 2,048 (ptuple-2048-pairs-2048-prices)"),
    ("ptuple", "reachable row window > 254 rows"): ("pair", "ptuple-rows-254-Reinforce", "ptuple-rows-255-Reinforce"),
    ("ptuple", "price grid too large for in-LDS policy tables"): ("pair", "ptuple-cdf-24KiB-ActorCritic", "ptuple-cdf-over-ActorCritic"),
    ("ptuple", "LUT image too large"): ("unreachable", "2,048 pairs need 51,200 B of the 64 KiB region"),
    ("ptuple", "one game does not fit LDS"): ("pair", "ptuple-lds-fits-Reinforce", "ptuple-lds-over-Reinforce"),
    ("mixed", "more than two discrete neural agents"): ("note", "a count, not a size"),
    ("mixed", "neural agent with more than 32 actions"): ("pair", "ptuple-nn-A32-Reinforce", "ptuple-nn-A33-Reinforce"),
    ("mixed", "QTable agent with more than 64 actions"): ("pair", "mixed-q-A64", "mixed-q-A65"),
    ("mixed", "tables and CAC networks of one game exceed 64 KiB of LDS"): ("pair", "mixed-64KiB-f32", "mixed-over-64KiB-f32"),
}


def word_bits_worst_case():
    """The widest action word over every 1-4 agents of 2..64 actions with at most 4,096 tuples (exhaustive)."""
    A = np.arange(2, 65, dtype=np.int64)
    bits = np.array([field_bits(int(x)) for x in A], np.int64)
    prod, width, worst = np.ones(1, np.int64), np.zeros(1, np.int64), 0
    for _ in range(4):
        prod = (prod[:, None] * A[None, :]).reshape(-1)
        width = (width[:, None] + bits[None, :]).reshape(-1)
        ok = prod <= 4096
        prod, width = prod[ok], width[ok]
        worst = max(worst, 1 + int(width.max()))
    return worst


def cases(plan=None, side=None):
    return [c for c in CASES if (plan is None or c["plan"] == plan) and (side is None or c["side"] == side)]


def expand(cs):
    """(case, dtype) pairs with pytest ids."""
    return [(c, dt) for c in cs for dt in c["dtypes"]]


def ids(pairs):
    return ["%s-%s" % (c["id"], dt) for c, dt in pairs]


__all__ = ["CASES", "BY_ID", "REASONS", "measure", "cases", "expand", "ids", "word_bits_worst_case"]
