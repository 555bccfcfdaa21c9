"""Parity mode of mixed games on the device (thrl_mixed.inj_*, MixedGameBatch.run(inj=...)): the reference's own runs
with a neural agent in the game (fixtures G12: QTable vs Reinforce = the shipped example_config.json, QTable vs
ActorCritic, Reinforce vs QTable with env noise), replayed from the recorded draws and sampled actions on each of the
three paths -- the general fused kernel (k_mixed_wave), the tuple-chain fused kernel (k_ptuple_episodes) and the
operator loop.  Trajectory, table, counter and epsilon are the reference's exactly; the network parameters within the
bounds stated at PARAM_SHARE / PARAM_STEP_MAX below; the three paths agree bit for bit."""
import functools

import numpy as np
import pytest

import mixed_injection_oracle as MO

pytestmark = pytest.mark.gpu

PATHS = ("wave", "tuple", "unfused")
# Network parameters after update k against the reference's: (i) fewer than 1 % of the elements off by more than 1e-5,
# the project's device-vs-oracle bound (test_gpu_nn.py); (ii) max |diff| <= k * 4.1e-4: G7's per-step bound
# (test_nn_oracle.py) -- an Adam step moves an element by at most lr = 2e-4 and a near-zero gradient can flip its sign --
# scaled by the number of steps.
PARAM_SHARE, PARAM_TOL, PARAM_STEP_MAX = 0.01, 1e-5, 4.1e-4


def _batch(fx, path, G, dtype="float64"):
    from th_rl_amd.mixed import MixedGameBatch
    d = fx.d
    mb = MixedGameBatch(fx.config, n_games=G, dtype=dtype, seed=3)
    q = np.zeros((G, mb.stride))
    o, (r, a) = mb.offsets[fx.qi], mb.shapes[fx.qi]
    q[:, o:o + r * a] = d["init_table"].ravel()
    mb.set_tables(q, np.full(G, float(d["state0"])))
    mb.nn[fx.ni].init().set_params(d["nn_w0"])
    mb.tuple_kernel = path == "tuple"
    return mb


def _snapshot(mb, fx):
    rb, b = mb.nn[fx.ni], mb.buf[fx.ni]
    return dict(q=mb.tables_numpy(), counter=mb.counters_numpy(), state=mb.states_numpy(), eps=list(mb.eps),
                count=list(mb.count), episode=mb.episode, step=rb.step, qoff=mb.offsets[fx.qi], params=rb.params.cpu().numpy(),
                adam_m=rb.adam_m.cpu().numpy(), adam_v=rb.adam_v.cpu().numpy(),
                ring={k: v.cpu().numpy() for k, v in b.items()})


def _run(mb, fx, path, inj, e0, e1):
    out = mb.run(e1 - e0, fused=path != "unfused", inj={k: v[e0:e1] for k, v in inj.items()})
    if path == "unfused":
        assert out["kernel"] == "unfused"
    else:
        assert out["kernel"] == "mixed-fused" and out["episode_kernel"] == path, (out["kernel"], out["episode_kernel"])
    return out


@functools.lru_cache(maxsize=None)
def _play(name, path, G, cuts=None, dtype="float64", upto=None):
    """One replay of fixture `name` in game index (2 if G > 2 else 0); the other games get other draws.  cuts: episodes
    at which a new run() call starts (default: one call).  Returns the snapshot after every call and the joined logs."""
    fx = MO.Fixture(name)
    game = 2 if G > 2 else 0
    E = fx.E if upto is None else upto
    inj = fx.inj(G, game)
    mb = _batch(fx, path, G, dtype)
    edges = [0] + [c for c in (cuts or ()) if 0 < c < E] + [E]
    snaps, rl, al = [], [], []
    for e0, e1 in zip(edges[:-1], edges[1:]):
        out = _run(mb, fx, path, inj, e0, e1)
        rl.append(out["game_reward_log"]); al.append(out["game_action_log"])
        snaps.append(_snapshot(mb, fx))
    return dict(fx=fx, game=game, edges=edges, snaps=snaps, rlog=np.concatenate(rl), alog=np.concatenate(al))


def _check_params(w, ref, k, what):
    diff = np.abs(w.astype(np.float64) - ref.astype(np.float64))
    share, worst = float((diff > PARAM_TOL).mean()), float(diff.max())
    print("%s: after update %d share(|diff| > 1e-5) = %.5f, max |diff| = %.3g" % (what, k, share, worst))
    assert share < PARAM_SHARE and worst <= k * PARAM_STEP_MAX, (what, k, share, worst)


def _check_against_fixture(res, path):
    fx, g, d = res["fx"], res["game"], res["fx"].d
    T, qi, ni = fx.T, fx.qi, fx.ni
    for e1, s in zip(res["edges"][1:], res["snaps"]):
        assert s["state"][g] == d["states"][e1 - 1, -1], (e1, s["state"][g])        # the price at each call boundary
        assert s["eps"][qi] == d["eps"][e1 - 1] and s["episode"] == e1
        n_upd = sum(1 for u in fx.updates if u < e1)
        assert s["step"] == n_upd
        # the neural agent's replay ring holds the steps since its last update (an update empties it logically; the slots
        # keep the transitions of the episodes before it): prices, actions and rewards of every step, exactly
        last = max([u + 1 for u in fx.updates if u < e1] + [0])
        first = last if last < e1 else max([u + 1 for u in fx.updates if u + 1 < e1] + [0])
        n = (e1 - first) * T
        assert s["count"][ni] == (e1 - last) * T
        assert np.array_equal(s["ring"]["nprice"][g, :n], d["states"][first:e1].ravel())
        assert np.array_equal(s["ring"]["price"][g, 1:n], d["states"][first:e1].ravel()[:-1])
        assert np.array_equal(s["ring"]["reward"][g, :n], d["rewards"][first:e1, :, ni].ravel())
        assert np.array_equal(s["ring"]["action"][g, :n], d["nn_action"][first:e1].ravel())
        if n_upd and fx.updates[n_upd - 1] == e1 - 1:                                # this call ended with update n_upd
            _check_params(s["params"][g], d["nn_w"][n_upd - 1], n_upd, "%s %s G=%d" % (fx.kind, path, len(s["state"])))
    E = res["edges"][-1]
    s = res["snaps"][-1]
    if E == fx.E:
        o, n = s["qoff"], d["final_table"].size
        assert np.array_equal(s["q"][g][o:o + n], d["final_table"].ravel())
        assert np.array_equal(s["counter"][g][o:o + n].astype(np.float64), d["final_counter"].ravel())
        _check_params(s["params"][g], d["nn_w"][-1], len(fx.updates), "%s %s final" % (fx.kind, path))
    if path == "unfused":
        assert np.array_equal(res["rlog"][:, :, g], d["rewards_log"][:E]) and np.array_equal(res["alog"][:, :, g], d["actions_log"][:E])
    else:                         # the log rows' contract
        np.testing.assert_allclose(res["rlog"][:, :, g], d["rewards_log"][:E], rtol=1e-12, atol=0)
        np.testing.assert_allclose(res["alog"][:, :, g], d["actions_log"][:E], rtol=1e-12, atol=0)


def _update_cuts(name):
    fx = MO.Fixture(name)
    return tuple(u + 1 for u in fx.updates)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sorted(MO.FIXTURES))
def test_one_game_reproduces_the_reference_run(name, path):
    """G = 1, float64 tables, one run() call per network update: the price at every call boundary, every step in the
    replay ring, epsilon, the final table and counter exactly; the parameters after each update within the bounds above."""
    _check_against_fixture(_play(name, path, 1, cuts=_update_cuts(name)), path)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sorted(MO.FIXTURES))
def test_fixture_game_among_other_games(name, path):
    """G = 4 in ONE run() call (the launches end at the updates by themselves), the fixture's game at index 2 and
    other draws in games 0, 1 and 3: a slip in the game index of any injected array shows here."""
    res = _play(name, path, 4)
    _check_against_fixture(res, path)
    s = res["snaps"][-1]
    assert not np.array_equal(s["q"][0], s["q"][2]) and not np.array_equal(s["q"][3], s["q"][2])


@pytest.mark.parametrize("G,cuts", [(1, "updates"), (4, None)])
@pytest.mark.parametrize("name", sorted(MO.FIXTURES))
def test_three_paths_agree_bit_for_bit(name, G, cuts):
    """General kernel == tuple-chain kernel == operator loop on everything a run leaves behind: tables, counters,
    states, logs, replay rings, network parameters and Adam moments -- as without injection."""
    cuts = _update_cuts(name) if cuts else None
    ref = _play(name, "unfused", G, cuts=cuts)
    for path in ("wave", "tuple"):
        res = _play(name, path, G, cuts=cuts)
        assert np.array_equal(res["rlog"], ref["rlog"]) and np.array_equal(res["alog"], ref["alog"]), path
        for a, b in zip(res["snaps"], ref["snaps"]):
            for k in ("q", "counter", "state", "params", "adam_m", "adam_v"):
                assert np.array_equal(a[k], b[k]), (path, k)
            assert (a["eps"], a["count"], a["episode"], a["step"]) == (b["eps"], b["count"], b["episode"], b["step"]), path
            for k in a["ring"]:
                assert np.array_equal(a["ring"][k], b["ring"][k]), (path, "ring", k)


@pytest.mark.parametrize("path", PATHS)
def test_split_off_an_update_boundary_gives_the_same_bits(path):
    """Two run() calls cut at episode 13 (updates fall at 9, 19, 29) == one call."""
    one, two = _play("reinforce", path, 4), _play("reinforce", path, 4, cuts=(13,))
    assert np.array_equal(one["rlog"], two["rlog"]) and np.array_equal(one["alog"], two["alog"])
    a, b = one["snaps"][-1], two["snaps"][-1]
    for k in ("q", "counter", "state", "params", "adam_m", "adam_v"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["eps"], a["count"], a["episode"], a["step"]) == (b["eps"], b["count"], b["episode"], b["step"])
    for k in a["ring"]:
        assert np.array_equal(a["ring"][k], b["ring"][k]), k


@pytest.mark.parametrize("path", PATHS)
def test_float32_tables_follow_the_float64_run_for_five_episodes(path):
    """float32 tables: the same prices as the float64 reference for the first 5 episodes (test_gpu_parity.py's window)."""
    res = _play("reinforce", path, 1, dtype="float32", upto=5)
    fx, d, s = res["fx"], res["fx"].d, res["snaps"][-1]
    assert s["state"][0] == d["states"][4, -1]
    assert np.array_equal(s["ring"]["nprice"][0, :5 * fx.T], d["states"][:5].ravel())
    np.testing.assert_allclose(res["rlog"][:, :, 0], d["rewards_log"][:5], rtol=1e-12, atol=0)


@pytest.mark.parametrize("path", PATHS)
def test_injected_action_outside_the_grid_counts_as_the_last_action(path):
    """An injected action that is none of the agent's is data the host cannot see: it is clamped to the last action."""
    fx = MO.Fixture("noise_swapped")
    E, G = 2, 2
    good = fx.inj(G, 0, 0, E)
    sel = np.zeros(good["action"][:, :, fx.ni, :].shape, bool); sel[:, ::3, :] = True
    bad = {k: v.copy() for k, v in good.items()}
    good["action"][:, :, fx.ni, :][sel] = fx.A - 1
    bad["action"][:, :, fx.ni, :][sel] = np.where(np.arange(sel.sum()) % 2, 100, -3).astype(np.int8)
    if path != "unfused":               # the fused kernels clamp the QTable agent's random choice in the same way
        Aq = int(fx.config["agents"][fx.qi]["actions"])
        good["choice"][:, 1::3, fx.qi, :] = Aq - 1
        bad["choice"][:, 1::3, fx.qi, :] = 90
    snaps = []
    for inj in (good, bad):
        mb = _batch(fx, path, G)
        _run(mb, fx, path, inj, 0, E)
        snaps.append(_snapshot(mb, fx))
    for k in ("q", "counter", "state", "params"):
        assert np.array_equal(snaps[0][k], snaps[1][k]), k
    assert np.array_equal(snaps[0]["ring"]["action"][:, :E * fx.T] == fx.A - 1, snaps[1]["ring"]["action"][:, :E * fx.T] == fx.A - 1)
    assert snaps[1]["ring"]["action"].max() == fx.A - 1 and snaps[1]["ring"]["action"].min() >= 0


def test_library_rejects_a_partial_set_on_the_device():
    """run() builds complete sets only; a caller of the C entry point that leaves a stream out gets THRL_ERR_BAD_CONFIG
    and nothing is launched (the tables stay as they were)."""
    from th_rl_amd import mixed
    from th_rl_amd._lib import ERR_BAD_CONFIG, ThrlError
    fx = MO.Fixture("reinforce")
    mb = _batch(fx, "wave", 1)
    q0 = mb.tables_numpy().copy()
    inj = mixed.check_injection(fx.inj(1, 0, 0, 2), 2, fx.T, 2, 1, mb.kinds, False)
    del inj["action"]
    with pytest.raises(ThrlError) as ei:
        mb._run_fused(2, inj=inj)
    assert ei.value.code == ERR_BAD_CONFIG and "inj_action" in str(ei.value)
    assert np.array_equal(mb.tables_numpy(), q0) and mb.episode == 0
