"""Host side of the parity mode of mixed games (thrl_mixed.inj_*, MixedGameBatch.run(inj=...)): the composed oracle fed
the reference's recorded draws and sampled actions reproduces the reference runs of fixtures G12; the struct mirror;
the argument checks of run().  No GPU."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mixed_injection_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(MO.FIXTURES))
def test_composed_oracle_reproduces_reference_run(name):
    """Prices, rewards, log rows, epsilon, the final table and counter exactly; the network parameters after each
    update within 1e-6 (measured <= 6e-8 over 5 chained updates and 3 seeds when the bound was set; the margin allows
    for another BLAS summation order)."""
    fx = MO.Fixture(name)
    d = fx.d
    out = MO.composed_oracle(fx.config, d["init_table"], float(d["state0"]), d["nn_w0"], fx.inj())
    assert np.array_equal(out["prices"], d["states"])
    assert np.array_equal(out["rewards"], d["rewards"])
    assert np.array_equal(out["scaled"], d["scaled_actions"])
    assert np.array_equal(out["rewards_log"], d["rewards_log"])
    assert np.array_equal(out["actions_log"], d["actions_log"])
    assert np.array_equal(out["eps"], d["eps"])
    assert np.array_equal(out["table"], d["final_table"])
    assert np.array_equal(out["counter"].astype(np.float64), d["final_counter"])
    assert out["updates"] == fx.updates and len(fx.updates) >= 2
    for k in range(len(fx.updates)):
        diff = np.abs(out["nn_w"][k].astype(np.float64) - d["nn_w"][k].astype(np.float64))
        print("%s update %d: max |diff| %.3g" % (name, k + 1, diff.max()))
        assert diff.max() <= 1e-6, (k, float(diff.max()))


def test_fixtures_cover_what_they_are_for():
    r, a, n = MO.Fixture("reinforce"), MO.Fixture("actorcritic"), MO.Fixture("noise_swapped")
    assert (r.kind, r.qi, r.E, r.T, r.updates) == ("Reinforce", 0, 30, 100, [9, 19, 29]) and not r.noise
    assert (a.kind, a.qi, a.T) == ("ActorCritic", 0, 100) and len(a.updates) >= 2 and a.d["nn_w"].shape[1] == 5909 + 257
    assert (n.kind, n.qi, n.E, n.T) == ("Reinforce", 1, 8, 25) and n.noise
    assert (n.d["noise_u"] < 0.5).sum() > 20 and np.isfinite(n.d["noise_a"][n.d["noise_u"] < 0.5]).all()
    assert (r.d["choice"] >= 0).sum() > 1000 and (r.d["choice"][r.d["u"] >= 0.5] == -1).all()
    for fx in (r, a, n):
        assert fx.d["nn_action"].min() >= 0 and fx.d["nn_action"].max() < fx.A
    for f in MO.FIXTURES.values():                          # no fixture larger than the largest committed before (509 KB)
        assert os.path.getsize(os.path.join(MO.GOLDEN, f)) < 509 * 1024


def test_thrl_mixed_mirror_matches_the_header():
    """sizeof(thrl_mixed) and the offsets of the injection fields agree between include/thrl.h and _lib.Mixed."""
    from th_rl_amd import _lib
    fields = ["flags", "inj_u", "inj_choice", "inj_noise_u", "inj_noise_a", "inj_action"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "thrl.h"\nint main(){printf("%zu"' + "".join(' " %zu"' for _ in fields)
           + ',sizeof(thrl_mixed)' + "".join(",offsetof(thrl_mixed,%s)" % f for f in fields) + ');return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = list(map(int, subprocess.check_output([os.path.join(d, "s")]).split()))
    assert got == [ctypes.sizeof(_lib.Mixed)] + [getattr(_lib.Mixed, f).offset for f in fields]
    assert _lib.Mixed.inj_action.offset + 8 == ctypes.sizeof(_lib.Mixed)          # the last field: older callers' zeroed tail
    mx = _lib.Mixed()
    assert all(getattr(mx, f) is None for f in fields[1:])                       # zero-initialised = no injection


def test_abi_version_is_unchanged():
    from th_rl_amd import build, _lib
    build.build()
    assert _lib.load().thrl_version() == 4


KINDS = ["QTable", "Reinforce"]


def _arrays(E=3, T=5, N=2, G=4, noise=False):
    inj = dict(u=np.zeros((E, T, N, G)), choice=np.zeros((E, T, N, G), np.int8), action=np.zeros((E, T, N, G), np.int8))
    if noise:
        inj.update(noise_u=np.zeros((E, T, G)), noise_a=np.zeros((E, T, G)))
    return inj


def test_check_injection_shapes_and_partial_sets():
    from th_rl_amd._lib import ThrlError
    from th_rl_amd.mixed import check_injection
    out = check_injection(_arrays(), 3, 5, 2, 4, KINDS, False)
    assert sorted(out) == ["action", "choice", "u"]
    assert out["u"].dtype == np.float64 and out["choice"].dtype == np.int8 and out["action"].dtype == np.int8
    assert all(v.flags["C_CONTIGUOUS"] for v in out.values())
    assert sorted(check_injection(_arrays(noise=True), 3, 5, 2, 4, KINDS, True)) == ["action", "choice", "noise_a", "noise_u", "u"]
    # a stream the game does not consume may be absent: no QTable agent -> no u / choice; no neural agent -> no action
    assert sorted(check_injection(dict(action=np.zeros((3, 5, 2, 4), np.int8)), 3, 5, 2, 4, ["Reinforce", "ActorCritic"], False)) == ["action"]
    both = _arrays(); del both["action"]
    assert sorted(check_injection(both, 3, 5, 2, 4, ["QTable", "QTable"], False)) == ["choice", "u"]
    # int64 actions as the fixture generator's lists give them are taken when they fit int8
    wide = _arrays(); wide["action"] = wide["action"].astype(np.int64)
    assert check_injection(wide, 3, 5, 2, 4, KINDS, False)["action"].dtype == np.int8
    for key in ("u", "choice", "action"):                   # partial sets
        part = _arrays(); del part[key]
        with pytest.raises(ThrlError, match="all or nothing.*%s" % key):
            check_injection(part, 3, 5, 2, 4, KINDS, False)
    for key in ("noise_u", "noise_a"):
        part = _arrays(noise=True); del part[key]
        with pytest.raises(ThrlError, match="all or nothing.*%s" % key):
            check_injection(part, 3, 5, 2, 4, KINDS, True)
    with pytest.raises(ThrlError, match="all or nothing"):
        check_injection(_arrays(), 3, 5, 2, 4, KINDS, True)            # noise on, no noise arrays
    for key in ("u", "choice", "action"):                   # wrong shapes: episodes, steps, agents, games
        for shape in ((2, 5, 2, 4), (3, 4, 2, 4), (3, 5, 1, 4), (3, 5, 2, 3), (3, 5, 4, 2), (3, 5, 8)):
            bad = _arrays(); bad[key] = np.zeros(shape, bad[key].dtype)
            with pytest.raises(ThrlError, match=r"%r must have shape \[E,T,N,G\]" % key):
                check_injection(bad, 3, 5, 2, 4, KINDS, False)
    bad = _arrays(noise=True); bad["noise_a"] = np.zeros((3, 5, 2, 4))
    with pytest.raises(ThrlError, match=r"'noise_a' must have shape \[E,T,G\]"):
        check_injection(bad, 3, 5, 2, 4, KINDS, True)
    with pytest.raises(ThrlError, match="unknown injection key"):
        check_injection(dict(_arrays(), actions=1), 3, 5, 2, 4, KINDS, False)
    with pytest.raises(ThrlError, match="dict"):
        check_injection(np.zeros(3), 3, 5, 2, 4, KINDS, False)
    with pytest.raises(ThrlError, match="int8"):
        check_injection(dict(_arrays(), action=np.full((3, 5, 2, 4), 300)), 3, 5, 2, 4, KINDS, False)
    with pytest.raises(ThrlError, match="CAC"):
        check_injection(_arrays(), 3, 5, 2, 4, ["QTable", "CAC"], False)


def test_run_checks_injection_before_it_touches_the_device():
    """MixedGameBatch.run validates `inj` first: on a batch object that has no device state at all (no GPU here) a bad
    set raises the shape / partial-set error on every path, and nothing else is reached."""
    from th_rl_amd._lib import Cfg, ThrlError
    from th_rl_amd.mixed import MixedGameBatch
    mb = MixedGameBatch.__new__(MixedGameBatch)
    mb.T, mb.N, mb.G, mb.kinds, mb.cfg = 5, 2, 4, list(KINDS), Cfg()
    for fused in (None, True, False):
        with pytest.raises(ThrlError, match="must have shape"):
            mb.run(2, fused=fused, inj=_arrays())                      # arrays are for 3 episodes
        part = _arrays(); del part["action"]
        with pytest.raises(ThrlError, match="all or nothing"):
            mb.run(3, fused=fused, inj=part)
    mb.cfg.noise_prob = 0.5
    with pytest.raises(ThrlError, match="all or nothing.*noise_u, noise_a"):
        mb.run(3, inj=_arrays())


def _probe(lib, kinds, inj_fields, noise=0.0):
    """thrl_mixed_episodes on a config whose validation fails or passes before any launch: fake non-NULL pointers are
    never dereferenced on the paths taken here (every call returns from the injection checks)."""
    from th_rl_amd import _lib
    ag = dict(name="QTable", gamma=0.95, actions=21, states=100, action_range=[0.2, 0.4])
    slot = dict(name="QTable", states=1, actions=21, action_range=[0.2, 0.4], capacity=1, min_memory=1)
    cfg, _ = _lib.cfg_from_config({"agents": [ag if k == 0 else slot for k in kinds],
                                   "environment": dict(name="NoisyPriceState", noise_prob=noise, a=10, b=1, nplayers=2, max_steps=10)}, 2, 1)
    mx = _lib.Mixed()
    fake = 4096
    for i, k in enumerate(kinds):
        mx.kind[i] = k
        if k:
            mx.nn_params[i] = fake
    for f in inj_fields:
        setattr(mx, "inj_" + f, fake)
    r = _lib.Run(); r.n_episodes = 1
    rc = lib.thrl_mixed_episodes(ctypes.byref(cfg), ctypes.byref(mx), fake, None, fake, ctypes.byref(r), fake, fake, None)
    return rc, lib.thrl_last_error().decode()


def test_entry_point_rejects_partial_sets_and_cac():
    from th_rl_amd import build, _lib
    build.build()
    lib = _lib.load()
    for kinds, fields, noise, word in (([0, 1], ["u", "choice"], 0.0, "inj_action"),
                                       ([0, 1], ["action"], 0.0, "inj_u"),
                                       ([0, 1], ["u", "action"], 0.0, "inj_choice"),
                                       ([0, 2], ["choice", "action"], 0.0, "inj_u"),
                                       ([1, 2], ["u", "choice"], 0.0, "inj_action"),
                                       ([1, 0], ["u", "choice", "action"], 0.5, "inj_noise"),
                                       ([1, 0], ["u", "choice", "action", "noise_u"], 0.5, "inj_noise"),
                                       ([0, 0], ["noise_u", "noise_a"], 0.5, "inj_u")):
        rc, msg = _probe(lib, kinds, fields, noise)
        assert rc == _lib.ERR_BAD_CONFIG and word in msg, (kinds, fields, rc, msg)
    rc, msg = _probe(lib, [0, 3], ["u", "choice", "action"])
    assert rc == _lib.ERR_UNSUPPORTED and "CAC" in msg, (rc, msg)
