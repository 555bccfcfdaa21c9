"""tests/policy_reference.py (the float64 mirror of the device policy and its derived bounds) against the
reference-generated probabilities (fixtures G7 / G8) and against oracle/nn_oracle.py, the numpy float32 restatement:
the mirror's probabilities, the sampling window, the decisive draws and the argmax set, over the action counts and
weight regimes the GPU tests use -- so the bounds those tests hold the device to are shown to hold for an independent
float32 evaluation, and the decisive draws are shown to be there (the GPU tests are not vacuous)."""
import os

import numpy as np
import pytest

import policy_reference as PR
from oracle import nn_oracle as NN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REGIMES = ("init", "x8", "x40", "uniform", "ties")


@pytest.mark.parametrize("tag", ["cfg", "ent"])
def test_mirror_matches_reference_probabilities(tag):
    d = np.load(os.path.join(GOLDEN, "g7_reinforce.npz"))
    for wk, pk in (("_w0", "_probe_prob0"), ("_c1_w", "_probe_prob2")):
        p, _ = PR.probs64(d[tag + wk], 21, d[tag + "_probe_price"])
        np.testing.assert_allclose(p, d[tag + pk], rtol=2e-5, atol=1e-8)
    a = np.load(os.path.join(GOLDEN, "g8_actorcritic.npz"))
    A = {"cfg": 21, "ent": 15}[tag]
    p, _ = PR.probs64(a[tag + "_w0"], A, a[tag + "_probe_price"], value_head=True)
    np.testing.assert_allclose(p, a[tag + "_probe_prob0"], rtol=2e-5, atol=1e-8)
    assert np.array_equal(PR.probs64(a[tag + "_c1_w"], A, a[tag + "_probe_price"], value_head=True)[0].argmax(axis=1),
                          a[tag + "_probe_greedy2"])


def _cases(A, value_head, G=24):
    rs = np.random.RandomState(1000 * A + value_head)
    w0 = PR.host_init(G, A, value_head, rs)
    price = PR.probe_prices(G, rs)
    for name, (w, init_scale) in PR.regimes(w0, A).items():
        p64, S = PR.probs64(w, A, price, value_head=value_head)
        yield name, w, price, p64, PR.prob_bound(p64, S, init_scale=init_scale), rs


@pytest.mark.parametrize("value_head", [False, True])
@pytest.mark.parametrize("A", PR.A_GRID)
def test_float32_oracle_within_the_bound_window_and_decisive_draws(A, value_head):
    Pp = PR.n_policy_params(A)
    worst = 0.0
    for name, w, price, p64, bound, rs in _cases(A, value_head):
        G = len(price)
        assert np.abs(p64.sum(axis=1) - 1).max() < 1e-14
        p32 = np.stack([NN.forward(w[g, :Pp], A, [price[g]])[0][0] for g in range(G)])
        ratio = np.abs(p32.astype(np.float64) - p64) / bound
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, (name, float(ratio.max()))
        # greedy: the float32 argmax could be the maximum within the bound
        am = PR.argmax_set(p64, bound)
        assert am[np.arange(G), p32.argmax(axis=1)].all(), name
        assert am[np.arange(G), p64.argmax(axis=1)].all()
        # random draws: the float32 inverse CDF lands in the window
        for rep in range(8):
            u = rs.uniform(0, 1, G)
            a = np.array([NN.sample_action(w[g, :Pp], A, [price[g]], [u[g]])[0] for g in range(G)])
            win = PR.window(p64, bound, u.astype(np.float32))
            assert win[np.arange(G), a].all(), (name, rep)
            assert win.any(axis=1).all()
        # decisive draws: three per action with p_k > 8 tau, each admits exactly that action, the oracle takes it
        for g in range(G):
            draws, acts = PR.decisive_draws(p64[g], bound[g])
            ks = PR.decisive_actions(p64[g], bound[g])
            assert ks.size >= 1 and p64[g, ks].sum() > 0.5, (name, g, ks)        # the likely actions are all covered
            assert np.array_equal(np.bincount(acts, minlength=A)[ks], np.full(ks.size, 3))
            u32 = draws.astype(np.float32)
            assert np.all(np.diff(u32.reshape(-1, 3), axis=1) > 0), (name, g)     # three distinct float32 draws per action
            win = PR.window(np.broadcast_to(p64[g], (len(u32), A)), np.broadcast_to(bound[g], (len(u32), A)), u32)
            assert np.array_equal(win.sum(axis=1), np.ones(len(u32), int)) and win[np.arange(len(u32)), acts].all(), (name, g)
            got = NN.sample_action(w[g, :Pp], A, np.full(len(draws), price[g]), draws)
            assert np.array_equal(got, acts), (name, g)
        if name == "uniform":
            assert np.array_equal(PR.decisive_actions(p64[0], bound[0]), np.arange(A))
        if name == "ties":
            tied = PR.planted_ties(w, A)[1]
            for g in range(G):
                assert p32[g].argmax() == min(tied[g]) and NN.greedy_action(w[g, :Pp], A, [price[g]])[0] == min(tied[g])
                assert set(np.flatnonzero(am[g])) == set(tied[g]), (g, tied[g])
    print("A=%d value_head=%d: worst |dp| / bound of the float32 oracle %.3f" % (A, value_head, worst))


def test_window_edges():
    """The window's rule at its edges, on an exactly representable policy: p = 1/4 each, bound 0."""
    p = np.full((1, 4), 0.25); b = np.zeros((1, 4))
    f = np.float32
    # (the summation term (k + 1) u C_k stays: a draw exactly on a boundary admits both neighbours)
    for u, want in ((0.0, [0]), (0.25, [0, 1]), (0.2500002, [1]), (0.4999, [1]), (0.75, [2, 3]), (0.7500002, [3]), (1.0, [3])):
        assert list(np.flatnonzero(PR.window(p, b, np.array([u], f))[0])) == want, u
    # a positive bound widens both sides of a boundary, and only there
    b = np.full((1, 4), 1e-3)
    assert list(np.flatnonzero(PR.window(p, b, np.array([0.2505], f))[0])) == [0, 1]
    assert list(np.flatnonzero(PR.window(p, b, np.array([0.2495], f))[0])) == [0, 1]
    assert list(np.flatnonzero(PR.window(p, b, np.array([0.26], f))[0])) == [1]
    assert list(np.flatnonzero(PR.argmax_set(np.array([[0.5, 0.499, 0.001]]), np.full((1, 3), 1e-3))[0])) == [0, 1]
    with pytest.raises(AssertionError):
        PR.window(p, b, np.array([0.3]))                                    # a float64 draw: not what the kernels compare


def test_tie_sets_cover_the_ends_and_every_row_edge():
    for A in PR.A_GRID:
        sets = PR.tie_sets(A)
        assert (0, A - 1) in sets and all(max(s) < A and len(set(s)) == len(s) for s in sets)
        for edge in (8, 16, 24):
            assert ((edge - 1, edge) in sets) == (A > edge)
        assert A < 3 or any(len(s) == 3 for s in sets)
