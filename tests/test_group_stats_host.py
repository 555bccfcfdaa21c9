"""Host side of the per-group statistics (training.group_stats, th_rl_amd.group_stats): group assignment, the shard
cut of group ids, default ranges, the quantile formula, the exact shard merge and the utils readers.  No GPU."""
import json
import os

import numpy as np
import pytest

from th_rl_amd import group_stats as gs
from th_rl_amd.launch import shard_training

AG = dict(name="QTable", gamma=0.95, actions=21, states=100, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
CFG = {"agents": [dict(AG), dict(AG)], "environment": dict(ENV)}
GOLDEN_CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_run_example_config", "config.json")


def test_groups_from_sweep_first_appearance():
    ids, ng, values = gs.assign_groups(6, sweep={"gamma": [0.9, 0.35, 0.9, 0.5, 0.35, 0.9]})
    assert ng == 3 and ids.tolist() == [0, 1, 0, 2, 1, 0]
    assert values == [{"gamma": 0.9}, {"gamma": 0.35}, {"gamma": 0.5}]


def test_groups_from_sweep_agent_rows_and_several_keys():
    g = [[0.9, 0.9, 0.5, 0.5], [0.9, 0.5, 0.5, 0.9]]              # [N, G]: a combination is over agents too
    ids, ng, values = gs.assign_groups(4, sweep={"gamma": g, "noise_prob": [0.0, 0.0, 0.0, 0.1]})
    assert ids.tolist() == [0, 1, 2, 3] and ng == 4
    assert values[1] == {"gamma": [0.9, 0.5], "noise_prob": 0.0}
    ids, ng, _ = gs.assign_groups(4, sweep={"gamma": [[0.9, 0.9, 0.5, 0.9], [0.1, 0.1, 0.2, 0.1]]})
    assert ids.tolist() == [0, 0, 1, 0] and ng == 2
    # [G] is the same value for every agent
    a, _, _ = gs.assign_groups(4, sweep={"gamma": [0.9, 0.5, 0.9, 0.5]})
    b, _, _ = gs.assign_groups(4, sweep={"gamma": [[0.9, 0.5, 0.9, 0.5]] * 2})
    assert a.tolist() == b.tolist()


def test_no_sweep_is_one_group():
    ids, ng, values = gs.assign_groups(5)
    assert ng == 1 and ids.tolist() == [0] * 5 and values == [{}]


def test_explicit_groups_validated():
    ids, ng, _ = gs.assign_groups(4, groups=[2, 0, 2, 1])
    assert ng == 3 and ids.tolist() == [2, 0, 2, 1]
    assert gs.assign_groups(4, groups=[0, 0, 0, 0], n_groups=5)[1] == 5
    with pytest.raises(ValueError):
        gs.assign_groups(4, groups=[0, 1, 2])
    with pytest.raises(ValueError):
        gs.assign_groups(3, groups=[0, -1, 2])
    with pytest.raises(ValueError):
        gs.assign_groups(3, groups=[0, 4, 2], n_groups=3)
    with pytest.raises(ValueError):
        gs.GroupSpec(2, [0, 3], 2, gs.default_ranges(CFG))


def test_options():
    assert gs.parse_options(True)["bins"] == 256
    with pytest.raises(ValueError):
        gs.parse_options({"bins": 0})
    with pytest.raises(ValueError):
        gs.parse_options({"bins": 1025})
    with pytest.raises(ValueError):
        gs.parse_options({"binz": 3})


def _cfg(**training):
    return dict(CFG, training=dict({"seed": 1, "epochs": 2}, **training))


@pytest.mark.parametrize("world", [1, 2, 3])
def test_shard_training_global_group_ids(world):
    G = 10
    sw = {"gamma": [0.5, 0.5, 0.5, 0.5, 0.9, 0.5, 0.5, 0.5, 0.5, 0.35]}
    full, ng, _ = gs.assign_groups(G, sweep=sw)
    got = []
    for r in range(world):
        tr, off, n = shard_training(_cfg(n_games=G, sweep=sw, group_stats=True), r, world)
        assert tr["n_groups"] == ng == 3 and len(tr["groups"]) == n
        assert tr["group_stats"]["histograms"] is True and tr["group_stats"]["n_max"] == 8
        assert tr["groups"] == full[off:off + n].tolist()
        ids, ng_r, _ = gs.assign_groups(n, sweep=tr["sweep"], groups=tr["groups"], n_groups=tr["n_groups"])
        assert ng_r == 3
        got += ids.tolist()
    assert got == full.tolist()
    if world == 3:              # rank 0 (games 0-3) has no game of groups 1 and 2, and still knows 3 groups
        tr, _, _ = shard_training(_cfg(n_games=G, sweep=sw, group_stats=True), 0, 3)
        assert set(tr["groups"]) == {0} and tr["n_groups"] == 3


def test_shard_training_without_group_stats_is_unchanged():
    tr, _, _ = shard_training(_cfg(n_games=10), 0, 2)
    assert "groups" not in tr and "group_stats" not in tr


def test_default_ranges_shipped_config():
    cfg = json.load(open(GOLDEN_CFG))
    rng = gs.default_ranges(cfg)
    assert rng[0] == [0.0, 25.0] and rng[1] == [0.0, 25.0] and rng[4] == [0.0, 25.0]
    assert rng[2] == [0.2, 0.4] and rng[3] == [0.2, 0.4]
    assert gs.resolve_ranges(cfg, {"total": [5, 30], "action": [0, 1]})[2:] == [[0.0, 1.0], [0.0, 1.0], [5.0, 30.0]]
    with pytest.raises(ValueError):
        gs.resolve_ranges(cfg, {"price": [0, 1]})


def test_fixed_scales_bound():
    for lo, hi in ([0.0, 25.0], [-3.0, 7.5], [0.2, 0.4]):
        for n in (1, 1000, 1 << 20):
            s1, s2 = gs.fixed_scales([[lo, hi]], n)[0]
            M = 16 * max(abs(lo), abs(hi))
            assert s1 * M * n <= 2.0 ** 62 < 2 * s1 * M * n
            assert s2 * M * M * n <= 2.0 ** 62 < 2 * s2 * M * M * n


def test_quantiles_hand_computed():
    # one quantity, range [0, 4), 4 bins of width 1: bins 0 (under), 1..4, 5 (over)
    h = np.array([[0, 1, 2, 1, 0, 0]])              # values: one in [0,1), two in [1,2), one in [2,3)
    vmin, vmax = np.array([0.5]), np.array([2.5])
    q = gs.quantiles(h, vmin, vmax, [0.0, 0.25, 0.5, 0.75, 1.0], [0.0], [4.0])[0]
    # t = 1: first bin reaching 1 is bin 1 (cum 1): 0 + (1 - 0)/1 * 1 = 1.0
    # t = 2: bin 2 (cum 3): 1 + (2 - 1)/2 = 1.5;  t = 3: bin 2: 1 + (3 - 1)/2 = 2.0
    assert q.tolist() == [0.5, 1.0, 1.5, 2.0, 2.5]
    # clamped to [min, max]; targets in the under / overflow bins give the exact extremes
    h = np.array([[2, 0, 0, 0, 1, 1]])
    q = gs.quantiles(h, np.array([-7.0]), np.array([9.0]), [0.25, 0.5, 0.6, 0.9], [0.0], [4.0])[0]
    assert q.tolist() == [-7.0, -7.0, 3.4, 9.0]
    # empty cell
    assert np.isnan(gs.quantiles(np.zeros((1, 6), int), np.array([np.nan]), np.array([np.nan]), [0.5], [0.0], [4.0])).all()


def _desc(bins=8, n_max=16):
    spec = gs.GroupSpec(2, np.zeros(n_max, np.int32), 3, gs.default_ranges(CFG), bins=bins)
    return spec.describe()


def test_order_keys_and_min_max():
    x = np.array([-np.inf, -3.5, -0.0, 0.0, 1e-300, 2.0, 1e300])
    k = gs.order_key(x)
    assert (np.diff(k.astype(object)) > 0).all()
    assert np.array_equal(gs.key_value(k).view(np.uint64), x.view(np.uint64))
    mm = np.stack([~gs.order_key(np.array([-1.0, 4.0])), gs.order_key(np.array([3.0, 5.0]))], axis=-1)
    mm[1, 0] = 0
    vmin, vmax = gs.min_max(mm)
    assert vmin[0] == -1.0 and np.isnan(vmin[1]) and vmax.tolist() == [3.0, 5.0]


def test_merge_is_exact():
    rs = np.random.RandomState(2)
    G, E = 40, 3
    desc = _desc(n_max=G)
    ids = rs.randint(0, 3, G)
    r, a = rs.uniform(-1, 26, (E, 2, G)), rs.uniform(0, 1, (E, 2, G))
    full = gs.reduce_host(r, a, ids, 3, desc)
    cut = [0, 7, 7, 25, G]                          # includes an empty shard
    parts = [gs.reduce_host(r[:, :, lo:hi], a[:, :, lo:hi], ids[lo:hi], 3, desc) for lo, hi in zip(cut, cut[1:])]
    m = gs.merge(parts)
    for k in ("hist", "sums", "minmax"):
        assert np.array_equal(m[k], full[k]), k
    f = gs.finalize(full, desc)
    for k in range(3):
        sel = ids == k
        np.testing.assert_allclose(f["mean"][:, k, 0], r[:, 0, sel].mean(axis=1), rtol=1e-12)
        np.testing.assert_allclose(f["std"][:, k, 0], r[:, 0, sel].std(axis=1), rtol=1e-6)
        assert np.array_equal(f["min"][:, k, 4], (r[:, 0, sel] + r[:, 1, sel]).min(axis=1))


def test_host_mirror_bins():
    desc = _desc(bins=4)                             # reward range [0, 25): width 6.25
    r = np.array([[[-1.0, 0.0, 6.25, 24.999, 25.0, np.nan]]] * 2).reshape(1, 2, 6)
    a = np.zeros((1, 2, 6))
    h = gs.reduce_host(r, a, np.zeros(6, int), 3, desc)["hist"][0, 0, 0]
    assert h.tolist() == [1, 1, 1, 0, 1, 2]


def _write_run(d, desc, E, rs, n=2):
    os.makedirs(d, exist_ok=True)
    Q = 2 * n + 1
    ng = len(desc["groups"])
    json.dump(desc, open(os.path.join(d, "groups.json"), "w"))
    out = {}
    for f in ("mean", "std", "min", "max"):
        out[f] = rs.uniform(0, 1, (E, ng, Q))
        np.save(os.path.join(d, "group_%s.npy" % f), out[f])
    out["quantiles"] = np.sort(rs.uniform(0, 1, (E, ng, Q, 3)), axis=-1)
    np.save(os.path.join(d, "group_quantiles.npy"), out["quantiles"])
    return out


def test_utils_readers_on_synthetic_artefacts(tmp_path):
    from th_rl_amd import utils
    rs = np.random.RandomState(0)
    desc = _desc()
    exp = str(tmp_path / "exp")
    out = _write_run(exp, desc, 7, rs)
    json.dump(CFG, open(os.path.join(exp, "config.json"), "w"))
    gl = utils.group_log(exp, 2)
    assert list(gl.columns) == [("rewards", 0), ("rewards", 1), ("actions", 0), ("actions", 1)]
    assert np.array_equal(gl.to_numpy(), out["mean"][:, 2, :4])
    df = utils.group_quantiles(exp, 1)
    assert list(df.columns) == ["25th", "median", "75th", "Nash", "Cartel"]
    assert np.array_equal(df[["25th", "median", "75th"]].to_numpy(), out["quantiles"][:, 1, 4, :])
    assert abs(df["Nash"][0] - 200.0 / 9.0) < 1e-12 and df["Cartel"][0] == 25.0
    assert np.array_equal(utils.group_quantiles(exp, 0, "reward_1")["median"].to_numpy(), out["quantiles"][:, 0, 1, 1])
    with pytest.raises(KeyError):
        utils.group_log(str(tmp_path / "nothing"), 0)


def test_utils_readers_merge_shards(tmp_path):
    from th_rl_amd import utils
    rs = np.random.RandomState(1)
    G, E = 30, 4
    desc = _desc(n_max=G)
    ids = rs.randint(0, 3, G)
    r, a = rs.uniform(0, 25, (E, 2, G)), rs.uniform(0, 1, (E, 2, G))
    exp = tmp_path / "exp"
    for s, (lo, hi) in enumerate(((0, 12), (12, G))):
        d = exp / ("shard%d" % s)
        os.makedirs(d)
        raw = gs.reduce_host(r[:, :, lo:hi], a[:, :, lo:hi], ids[lo:hi], 3, desc)
        f = gs.finalize(raw, desc)
        json.dump(desc, open(d / "groups.json", "w"))
        for k in ("min", "max"):
            np.save(d / ("group_%s.npy" % k), f[k])
        np.save(d / "group_sums.npy", raw["sums"])
        np.save(d / "group_hist.npy", raw["hist"])
        (d / "shard_config.json").write_text(json.dumps(CFG))
    want = gs.finalize(gs.reduce_host(r, a, ids, 3, desc), desc)
    assert np.array_equal(utils.group_log(str(exp), 1).to_numpy(), want["mean"][:, 1, :4])
    assert np.array_equal(utils.group_quantiles(str(exp), 2)["median"].to_numpy(), want["quantiles"][:, 2, 4, 1])
