"""k_nn_act (thrl_nn_act / thrl_ac_act: policy_load, policy_probs, policy_cdf, policy_pick, policy_act of
th_rl_amd/csrc/thrl_policy.h) against the float64 mirror tests/policy_reference.py -- never against another device
kernel.  Every action count at a dispatch edge (8|9, 24|25), at a DPP row edge (every 8 actions), odd ones (a half-empty
last weight pair) and 32 (all 64 lanes); Reinforce and ActorCritic (the value head behind the policy's parameters);
1, 5 and 259 games (four games per block: a tail of three); per-game weights at the initial scale, peaked (fc_pi x 8,
x 40: probabilities that underflow, flat CDF tails), exactly uniform, and with exact ties.  Each assertion is hard:
every probability within the derived bound, every sampled action in the mirror's window, the one admissible action at
every decisive draw, the lowest index of an exact tie."""
import ctypes

import numpy as np
import pytest

import policy_reference as PR

pytestmark = pytest.mark.gpu

GAMES = (1, 5, 259)
SENTINEL = -7.0
GUARD = 64
WORST = {}                      # APAD -> worst |dp| / bound seen on the device in this session


def _apad(A):
    return 8 if A <= 8 else (24 if A <= 24 else 32)


def _batch(kind, G, A, seed=3):
    from th_rl_amd.nn import ActorCriticBatch, ReinforceBatch
    return (ActorCriticBatch if kind == "ActorCritic" else ReinforceBatch)(G, actions=A, seed=seed).init()


class _Act:
    """thrl_nn_act / thrl_ac_act called on a batch with the prices uploaded once and a probability buffer that is
    pre-filled and longer than G * A, so that a write outside the game's own A entries shows."""

    def __init__(self, rb, price):
        import torch
        self.rb, self.torch = rb, torch
        self.price = rb._dev(np.asarray(price, np.float64), torch.float64).reshape(rb.G)
        self.fn = getattr(rb.L, rb._fn["act"])

    def __call__(self, u=None, probs=False):
        """u: None (greedy) or draws [J, G]: J launches.  Returns actions [J, G] (J = 1 for greedy), and with probs=True
        the probabilities [G, A] of the last launch."""
        rb, torch = self.rb, self.torch
        with torch.cuda.device(rb.device):
            d_u = None if u is None else rb._dev(np.asarray(u, np.float64).reshape(-1, rb.G), torch.float64)
            J = 1 if u is None else d_u.shape[0]
            out = torch.full((J, rb.G), -1, dtype=torch.int32, device=rb.device)
            pbuf = torch.full((rb.G * rb.A + GUARD,), SENTINEL, dtype=torch.float32, device=rb.device) if probs else None
            for j in range(J):
                rc = self.fn(rb.G, rb.A, rb._p(rb.params), rb._p(self.price), rb._p(None if u is None else d_u[j]),
                             rb._p(out[j]), rb._p(pbuf), rb._stream())
                assert rc == 0, rc
            a = out.cpu().numpy()
        if not probs:
            return a
        pb = pbuf.cpu().numpy()
        assert np.all(pb[rb.G * rb.A:] == np.float32(SENTINEL)), "probabilities written past the last game's A entries"
        return a, pb[:rb.G * rb.A].reshape(rb.G, rb.A)


def _check_probs(p, p64, bound, A, what):
    assert np.isfinite(p).all() and (p >= 0).all(), what                   # (no slot kept its pre-fill, none got a stray 0 or NaN)
    ratio = np.abs(p.astype(np.float64) - p64) / bound
    WORST[_apad(A)] = max(WORST.get(_apad(A), 0.0), float(ratio.max()))
    assert ratio.max() <= 1.0, (what, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
    rowsum = p.astype(np.float64).sum(axis=1)
    assert np.abs(rowsum - 1.0).max() <= A * 2 * PR.U, (what, float(np.abs(rowsum - 1.0).max()))


def _check_sampling(act, p64, bound, rs, what):
    G, A = p64.shape
    # 259 random draws per shape (and G of them at the smaller batches), each in the window
    n_rounds = -(-259 // G) if G < 259 else 1
    u = rs.uniform(0, 1, (n_rounds, G))
    a = act(u)
    for j in range(n_rounds):
        win = PR.window(p64, bound, u[j].astype(np.float32))
        assert ((a[j] >= 0) & (a[j] < A)).all(), what
        bad = np.flatnonzero(~win[np.arange(G), a[j]])
        assert bad.size == 0, (what, "game", bad[:4], "draw", u[j][bad[:4]], "got", a[j][bad[:4]],
                               "admissible", [np.flatnonzero(win[b]) for b in bad[:4]])
    # decisive draws: launch j gives game g its j-th decisive draw (games with fewer repeat their first)
    dec = [PR.decisive_draws(p64[g], bound[g]) for g in range(G)]
    J = max(len(d[0]) for d in dec)
    assert min(len(d[0]) for d in dec) >= 3, what
    ud = np.stack([np.concatenate([d[0], np.full(J - len(d[0]), d[0][0])]) for d in dec], axis=1)
    want = np.stack([np.concatenate([d[1], np.full(J - len(d[1]), d[1][0])]) for d in dec], axis=1)
    got = act(ud)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "launch, game", bad[:4], "draw", [ud[i, g] for i, g in bad[:4]],
                           "got", [got[i, g] for i, g in bad[:4]], "want", [want[i, g] for i, g in bad[:4]])


@pytest.mark.parametrize("kind", ["Reinforce", "ActorCritic"])
@pytest.mark.parametrize("A", PR.A_GRID)
def test_act_kernel_against_the_float64_mirror(A, kind):
    vh = kind == "ActorCritic"
    Pp = PR.n_policy_params(A)
    for G in GAMES:
        rs = np.random.RandomState(10000 * G + 10 * A + vh)
        rb = _batch(kind, G, A, seed=3 + G)
        w0 = rb.params.cpu().numpy().copy()
        assert rb.P == Pp + (257 if vh else 0) and (G == 1 or not np.array_equal(w0[0], w0[1]))
        price = PR.probe_prices(G, rs)
        act = _Act(rb, price)
        regimes = PR.regimes(w0, A)
        tied = PR.planted_ties(w0, A)[1]
        for name, (w, init_scale) in regimes.items():
            what = "%s A=%d G=%d %s" % (kind, A, G, name)
            rb.set_params(w)
            p64, S = PR.probs64(w, A, price, value_head=vh)
            bound = PR.prob_bound(p64, S, init_scale=init_scale)
            greedy, p = act(None, probs=True)
            _check_probs(p, p64, bound, A, what)
            am = PR.argmax_set(p64, bound)
            assert am[np.arange(G), greedy[0]].all(), (what, greedy[0], [np.flatnonzero(r) for r in am[:4]])
            _check_sampling(act, p64, bound, rs, what)
            if name == "uniform":
                assert np.array_equal(greedy[0], np.zeros(G, int)), what            # all tied: the lowest index
                assert np.all(p == np.float32(1.0) / np.float32(A)), what
                if A in (2, 8, 16, 32):
                    # p = 1/A and its running sums are exact in float32: action j covers [j/A, (j+1)/A), the rule is u < C
                    u = np.repeat((np.arange(A) / A)[:, None], G, axis=1)
                    assert np.array_equal(act(u), np.repeat(np.arange(A)[:, None], G, axis=1)), what
                    inside = np.repeat(((np.arange(A) + 1) / A * (1 - 2.0 ** -24))[:, None], G, axis=1)   # the float32 below (j+1)/A
                    assert np.array_equal(act(inside), np.repeat(np.arange(A)[:, None], G, axis=1)), what
                    assert np.array_equal(act(np.zeros((1, G)))[0], np.zeros(G, int)), what
                    # Philox's largest draw rounds to 1.0f, which no cumulative probability exceeds: the last action
                    assert np.array_equal(act(np.full((1, G), 1 - 2.0 ** -32))[0], np.full(G, A - 1)), what
            if name == "ties":
                low = np.array([min(t) for t in tied])
                assert np.array_equal(greedy[0], low), (what, greedy[0][:8], low[:8])
                for g in range(G):
                    assert np.unique(p[g, list(tied[g])]).size == 1 and set(np.flatnonzero(p[g] == p[g].max())) == set(tied[g]), (what, g)
        # the largest draw at non-uniform policies too: the fallback, or the last action whose running sum reaches 1
        for name in ("init", "x40"):
            w, init_scale = regimes[name]
            rb.set_params(w)
            p64, S = PR.probs64(w, A, price, value_head=vh)
            bound = PR.prob_bound(p64, S, init_scale=init_scale)
            u = np.full((1, G), 1 - 2.0 ** -32)
            a = act(u)[0]
            assert PR.window(p64, bound, u[0].astype(np.float32))[np.arange(G), a].all(), (kind, A, G, name, a[:8])
    print("worst |dp| / bound on the device so far, by APAD: %s" % {k: round(v, 4) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("A", PR.A_GRID)
def test_value_head_does_not_reach_the_policy_head(A):
    """ActorCritic's parameter stride includes fc_v, its policy parameters sit where Reinforce's do: with fc_v.weight and
    bias at 1e3 the probabilities and actions equal, bit for bit, those of a Reinforce batch given the same first Pp
    parameters -- and stay within the mirror's bound."""
    G = 259
    Pp = PR.n_policy_params(A)
    rs = np.random.RandomState(77 + A)
    ab = _batch("ActorCritic", G, A, seed=9)
    rb = _batch("Reinforce", G, A, seed=1)
    w0 = ab.params.cpu().numpy().copy()
    price = PR.probe_prices(G, rs)
    u = rs.uniform(0, 1, (3, G))
    for factor in (1, 8):
        w = PR.scale_head(w0, A, factor)
        ab.set_params(w)
        ref_greedy, ref_p = _Act(ab, price)(None, probs=True)
        ref_a = _Act(ab, price)(u)
        w[:, Pp:] = 1e3
        ab.set_params(w)
        rb.set_params(w[:, :Pp])
        acts, probs = [], []
        for b in (ab, rb):
            act = _Act(b, price)
            g_, p_ = act(None, probs=True)
            acts.append(np.concatenate([g_, act(u)])); probs.append(p_)
        assert np.array_equal(probs[0].view(np.uint32), probs[1].view(np.uint32)), (A, factor)
        assert np.array_equal(acts[0], acts[1])
        assert np.array_equal(probs[0].view(np.uint32), ref_p.view(np.uint32))          # nothing in the policy head changed
        assert np.array_equal(acts[0], np.concatenate([ref_greedy, ref_a]))
        p64, S = PR.probs64(w, A, price, value_head=True)
        _check_probs(probs[0], p64, PR.prob_bound(p64, S, init_scale=factor == 1), A, "value head 1e3, A=%d x%d" % (A, factor))
    print("worst |dp| / bound on the device so far, by APAD: %s" % {k: round(v, 4) for k, v in sorted(WORST.items())})
