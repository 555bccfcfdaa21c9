"""The analyses on tables wider than 256 actions: greedy policies that hold action indices no byte holds.

Random tables through set_tables (no training) whose rows have planted maxima at the last action, at 255, at 256 and at a
low index (wide_grids_cases.planted_tables): a policy staged in 8 bits where 16 are needed, or read with the wrong width,
plays another action and walks elsewhere.  Every output is held to the analysis's own numpy mirror bit for bit, through the
_check helper of that analysis's own GPU test, at the smallest shapes that take each path of its plan:

  thrl_deviation      one-byte staging (max_a = 256), two-byte staging (257), the lookup-table limit (sum of the action
                      counts 1,024 staged, 1,025 not) and the LDS budget (64 KiB of staged policy windows);
  thrl_crossplay      extraction and walk at 257 actions;     thrl_policy_track   at 257 actions;
  thrl_tuple_policy   (k_tp_qtable) at 257 x 15 tuples;
  thrl_attractors, thrl_equilibrium, thrl_stationary and the noise variants of the last two and of deviation at 257 x 15,
  the widest first agent the limit of 4,096 action tuples leaves beside a second agent worth the name."""
import numpy as np
import pytest

import stationary_mirror as S
import test_gpu_attractors as TA
import test_gpu_convergence as TC
import test_gpu_crossplay as TX
import test_gpu_deviation as TD
import test_gpu_deviation_noise as TDN
import test_gpu_equilibrium as TE
import test_gpu_equilibrium_noise as TEN
import test_gpu_stationary as TS
import wide_grids_cases as W

pytestmark = pytest.mark.gpu

G = 70                                      # one wave of games and a tail, for the kernels that give a game a wave
G_WALK = 300                                # a full block of 256 lanes and a tail, for the walks (one lane per game)


def _batch(config, dtype="float32", seed=1, n_games=G):
    from th_rl_amd.batched import GameBatch
    q = W.planted_tables(config, n_games, dtype, seed=seed)
    s0 = np.random.RandomState(seed).uniform(0, 10, n_games)
    return GameBatch(config, n_games=n_games, dtype=dtype, seed=seed).set_tables(q, s0)


def _plays_past(pol, bound):
    """The extracted policies do hold what the narrow field loses."""
    assert (np.asarray(pol).astype(np.int64) >= bound).sum() >= 5


# ------------------------------------------------------------------------------------------------ thrl_deviation
DEVIATION = {
    "one-byte-256": (W.game([W.agent(256, states=12), W.agent(21, states=30, gamma=0.9)], T=10), True, 1),
    "two-byte-257": (W.game([W.agent(257, states=12), W.agent(21, states=30, gamma=0.9)], T=10), True, 2),
    "21x257": (W.game([W.agent(21, states=30), W.agent(257, states=12, gamma=0.9)], T=10), True, 2),
    "lut-1024": (W.game([W.agent(1000, states=12), W.agent(24, states=30, gamma=0.9)], T=10), True, 2),
    "lut-1025": (W.game([W.agent(1000, states=12), W.agent(25, states=30, gamma=0.9)], T=10), False, 2),
    "lds-budget": (W.game([W.agent(257, states=1000), W.agent(21, states=1000, gamma=0.9)], T=10), False, 2),
}


def _deviation_plan(config):
    """(staged, bytes per staged policy entry) as thrl_deviation plans it (thrl_deviation.h: a tile of 256 games, 64 KiB of
    LDS, a scale table of at most 1,024 entries; tests/test_wide_grids_host.py reads those three constants and the
    plan's two expressions from the sources, so this copy fails there when they move)."""
    A = [a["actions"] for a in config["agents"]]
    lo, hi = [], []
    for a in config["agents"]:          # the reachable rows: prices between the lowest and the highest joint action
        lo.append(a["action_range"][0]); hi.append(a["action_range"][1])
    p_lo, p_hi = max(0.0, 10 - 10 * sum(hi)), 10 - 10 * sum(lo)
    entries = sum(int(np.rint(p_hi / 10 * a["states"])) - int(np.rint(p_lo / 10 * a["states"])) + 2 for a in config["agents"])
    pol_bytes = 1 if max(A) <= 256 else 2
    lds = ((sum(A) * 8 + 15) & ~15) + 256 * entries * pol_bytes
    return sum(A) <= 1024 and lds <= 64 * 1024, pol_bytes


@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("name", list(DEVIATION))
def test_deviation_on_every_staging_path(name, dtype):
    config, staged, pol_bytes = DEVIATION[name]
    assert _deviation_plan(config) == (staged, pol_bytes)
    n = G if name == "lds-budget" else G_WALK         # (278,000 table elements per game there: the mirror's time)
    gb = _batch(config, dtype, seed=3, n_games=n)
    A = [a["actions"] for a in config["agents"]]
    wide = int(np.argmax(A))
    _plays_past(S.policies(config, gb.tables_numpy()), min(255, max(A) - 1))
    out = TD._check(gb, config, deviator=wide, steps=6, dev_len=2, horizon=512)
    TD._check(gb, config, deviator=1 - wide, steps=5, dev_len=1, horizon=512)
    TD._check(gb, config, deviator=wide, steps=4, dev_len=2, action=A[wide] - 1, horizon=512,
              state0=np.linspace(0.0, 10.0, n))
    # the walk does play the planted columns: a scaled action of the wide agent that only an index past 254 gives
    lo, hi = config["agents"][wide]["action_range"]
    assert (out["action_rows"][:, wide] > lo + (hi - lo) * 254.5 / (A[wide] - 1)).sum() >= 5


# ------------------------------------------------------------------------------------------------ policies at 257
WIDE2 = W.game([W.agent(257, states=12), W.agent(21, states=30, gamma=0.9)], T=10)
WIDE2_SWAPPED = W.game([W.agent(21, states=30), W.agent(257, states=12, gamma=0.9)], T=10)


@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("config,n", [(WIDE2, G_WALK), (WIDE2_SWAPPED, G_WALK), (DEVIATION["lds-budget"][0], G)],
                         ids=["257x21", "21x257", "unstaged"])
def test_crossplay_extracts_and_walks_wide_policies(config, n, dtype):
    """"unstaged": a game's tables are past the extraction's LDS window and the policy windows past the walk's."""
    from th_rl_amd import crossplay as xp
    gb = _batch(config, dtype, seed=4, n_games=n)
    pol = xp.extract(gb).cpu().numpy().view(np.uint16)
    ref = S.policies(config, gb.tables_numpy())
    assert pol.shape == ref.shape and np.array_equal(pol, ref)
    _plays_past(pol, 256)
    TX._check(gb, config, TX._rotate(n, 1), steps=6, horizon=512, strangers=False)
    rs = np.random.RandomState(4)
    TX._check(gb, config, rs.randint(0, n, size=(2, 90)), state0=rs.uniform(0, 10, 90), steps=3, horizon=512, strangers=False)


@pytest.mark.parametrize("dtype", W.DTYPES)
def test_policy_track_on_wide_policies(dtype):
    import torch
    gb = _batch(WIDE2, dtype, seed=5)
    gb.episode = 3
    tr = gb.track_convergence(window=2, every=1)
    m = TC._mirror(gb, 2)
    TC._compare(tr, m, "baseline")
    _plays_past(m.arrays()["policy"].view(np.uint16), 256)
    q = gb.tables_numpy().copy()
    for e, (col, games) in zip((4, 5, 6, 7), ((256, slice(0, 20)), (255, slice(10, 30)), (256, slice(0, 5)), (3, slice(40, 41)))):
        q[games, col] = 50.0 + e                   # row 0 of agent 0: a new greedy action on either side of a byte
        q[60:, 255 + e % 2] = 100.0 + e            # restless games: 255, 256, 255, ... -- they never converge
        gb.q.copy_(torch.from_numpy(q))
        gb.episode = e
        assert tr.check() == m.check(q, e, state=gb.states_numpy())
        TC._compare(tr, m, "check at %d" % e)
    assert 0 < m.n_converged < G


@pytest.mark.parametrize("dtype", W.DTYPES)
def test_tuple_policy_of_a_wide_qtable(dtype):
    """k_tp_qtable at 257 x 15 tuples: entry t of an agent is its first argmax in the row of tuple t's price."""
    from th_rl_amd import tuple_play as tp
    gb = _batch(WIDE15, dtype, seed=6)
    pol = tp.extract(gb).cpu().numpy().view(np.uint16)
    price = tp.tables(WIDE15)["price"]
    assert pol.shape == (G, 2, 257 * 15) and price.shape == (257 * 15,)
    rows = S.policies(WIDE15, gb.tables_numpy())                   # [G, P]: every table row's greedy action
    off = 0
    for i, a in enumerate(WIDE15["agents"]):
        row = np.rint(price / 10.0 * a["states"]).astype(np.int64)          # encode64, half-even
        assert row.min() >= 0 and row.max() <= a["states"] and np.unique(row).size >= 3
        assert np.array_equal(pol[:, i, :], rows[:, off + row])
        off += a["states"] + 1
    _plays_past(pol[:, 0], 256)


# ------------------------------------------------------------------------------------------------ the state-set analyses
WIDE15 = W.game([W.agent(257, states=50), W.agent(15, states=40, gamma=0.9)], T=10)
GS = 21                                     # their mirrors walk every state of every game


def test_the_widest_pair_is_within_the_tuple_limit():
    from th_rl_amd import _lib
    assert 257 * 15 <= _lib.TP_MAX_TUPLES < 257 * 16


@pytest.mark.parametrize("dtype", W.DTYPES)
def test_attractors_on_wide_policies(dtype):
    gb = _batch(WIDE15, dtype, seed=7, n_games=GS)
    TA._check(gb, WIDE15)
    TA._check(gb, WIDE15, state0=np.linspace(0.5, 9.5, GS))


@pytest.mark.parametrize("dtype", W.DTYPES)
def test_equilibrium_on_wide_policies(dtype):
    gb = _batch(WIDE15, dtype, seed=8, n_games=GS)
    out = TE._check(gb, WIDE15)
    _plays_past(out["br_policy"][0], 256)       # the wide agent's best response needs the second byte


@pytest.mark.parametrize("dtype", W.DTYPES)
def test_stationary_on_wide_policies(dtype):
    gb = _batch(WIDE15, dtype, seed=9, n_games=GS)
    TS._check(gb, WIDE15, noise_prob=0.2)
    TS._check(gb, WIDE15, noise_prob=0.05, start="state")


def test_equilibrium_noise_on_wide_policies():
    gb = _batch(WIDE15, "float32", seed=10, n_games=GS)
    TEN._check(gb, WIDE15, noise_prob=0.2)


def test_deviation_noise_on_wide_policies():
    gb = _batch(WIDE15, "float32", seed=11, n_games=GS)
    TDN._check(gb, WIDE15, noise_prob=0.2, deviator=0, steps=6, dev_len=2)
    TDN._check(gb, WIDE15, noise_prob=0.2, deviator=0, steps=4, dev_len=1, action=256)
