"""Per-group learning-curve statistics (thrl_group_stats, include/thrl.h): for every epoch, group (one point of a
config sweep) and quantity, a histogram, fixed-point sums of x and x^2 and the exact min / max over the group's
games, reduced on the device from the per-game episode rows.  This is the distribution over runs that the
reference's analysis plots per config (utils.py plot_learning_curve_conf / plot_learning_curve_sweep /
plot_sweep_conf / plot_mean_conf).

Quantities, Q = 2N + 1 per game and episode: reward_i (i < N), action_i (i < N), total = sum_i reward_i.  The values
are the per-epoch ones.  The reference smooths each run's curve with ewm(halflife=1000) before its quantiles; that
smoothing is off by default and is asked for with the option "smooth" (a halflife): thrl_ewm_rows then smooths every
game's rows on the device (Smoother; pandas' ewm(halflife=h, adjust=True).mean(), except that a non-finite value is
not skipped as pandas skips a NaN: it makes that game's smoothed values non-finite from then on, and those land in the
overflow bin), the same reduction runs on the smoothed rows, and the run writes a second set of statistics under the
prefix "group_smooth".  Its "total" is the sum of the smoothed rewards in agent order.

Quantiles from the histogram: with n values in a cell and target t = q * n, take the first bin whose cumulative
count reaches t and interpolate linearly inside it, lower edge + (t - count below) / count in bin * bin width,
clamped to [min, max]: at most one bin width from the exact quantile.  q = 0 is the exact min and q = 1 the exact
max; a target that falls in the underflow or overflow bin returns the exact min or max.

Mean and std come from the integer sums: mean = S1 / s1 / n, std = sqrt(max(0, S2 / s2 / n - mean^2)) (population
std); each value enters S1 rounded to 1 / s1 (and x^2 to 1 / s2), so the mean is exact to 0.5 / s1.  They assume
finite values (a non-finite value counts in the overflow bin only, and in n).

Shards combine exactly (merge): hist and sums are added, minmax by element-wise max of the stored keys.
"""
import ctypes
import json
import math

import numpy as np

from . import _lib
from ._lib import ThrlError

DEFAULT_BINS = 256
DEFAULT_QUANTILES = (0.25, 0.5, 0.75)


def quantity_names(n_agents):
    n = int(n_agents)
    return ["reward_%d" % i for i in range(n)] + ["action_%d" % i for i in range(n)] + ["total"]


def parse_options(opt):
    """training.group_stats (true or a dict) -> the dict with every key filled in."""
    if opt is True:
        opt = {}
    if not isinstance(opt, dict):
        raise ValueError("training.group_stats must be true or a dict, got %r" % (opt,))
    known = {"bins", "quantiles", "histograms", "greedy_iters", "ranges", "n_max", "smooth"}
    bad = set(opt) - known
    if bad:
        raise ValueError("training.group_stats: unknown keys %s (known: %s)" % (sorted(bad), ", ".join(sorted(known))))
    out = dict(bins=DEFAULT_BINS, quantiles=list(DEFAULT_QUANTILES), histograms=False, greedy_iters=0, ranges={},
               n_max=None)
    out.update(opt)
    out["bins"] = int(out["bins"])
    if not 1 <= out["bins"] <= _lib.STATS_MAX_BINS:
        raise ValueError("training.group_stats.bins=%d out of [1, %d]" % (out["bins"], _lib.STATS_MAX_BINS))
    out["quantiles"] = [float(q) for q in out["quantiles"]]
    if any(not 0.0 <= q <= 1.0 for q in out["quantiles"]):
        raise ValueError("training.group_stats.quantiles must lie in [0, 1]")
    out["greedy_iters"] = int(out["greedy_iters"])
    out["histograms"] = bool(out["histograms"])
    if out.get("smooth") is None:       # off: the dict is what it was before the option existed
        out.pop("smooth", None)
    else:
        out["smooth"] = {"halflife": parse_halflife(out["smooth"])}
    return out


def parse_halflife(v):
    """training.group_stats.smooth (a number or {"halflife": h}) -> h as a float; finite and > 0."""
    if isinstance(v, dict):
        if set(v) - {"halflife", "decay"} or "halflife" not in v:
            raise ValueError("training.group_stats.smooth: a dict must be {\"halflife\": h}, got keys %s" % sorted(v))
        v = v["halflife"]
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError("training.group_stats.smooth must be a halflife (a number or {\"halflife\": h}), got %r" % (v,))
    h = float(v)
    if not (math.isfinite(h) and h > 0.0):
        raise ValueError("training.group_stats.smooth: halflife=%r must be finite and > 0" % (v,))
    return h


# ---------------------------------------------------------------------------------------------- groups
def _per_game(v, n_games):
    """A sweep array ([G] or [N, G]) as [rows, G] float64."""
    a = np.asarray(v, np.float64)
    if a.shape[-1:] != (n_games,):
        raise ValueError("sweep array of shape %r does not end in n_games=%d" % (a.shape, n_games))
    return a.reshape(-1, n_games)


def assign_groups(n_games, sweep=None, groups=None, n_groups=None):
    """(ids int32 [G], n_groups, values) for a run's games.  groups: explicit global group ids (a list of n_games
    ints >= 0; n_groups defaults to max + 1).  Otherwise with a sweep, one group per distinct combination of the
    per-game values over all keys and agents, numbered by first appearance in game order; values[k] is group k's
    {key: value ([G] arrays) or [value per agent] ([N, G] arrays)}.  Otherwise one group."""
    G = int(n_games)
    if groups is not None:
        ids = np.asarray(list(groups), dtype=np.int64).reshape(-1)
        if ids.size != G:
            raise ValueError("training.groups has %d entries for n_games=%d" % (ids.size, G))
        if ids.size and ids.min() < 0:
            raise ValueError("training.groups: negative group id %d" % int(ids.min()))
        top = int(ids.max()) + 1 if ids.size else 1
        ng = top if n_groups is None else int(n_groups)
        if ng < top:
            raise ValueError("training.groups: id %d out of range for n_groups=%d" % (top - 1, ng))
        return ids.astype(np.int32), ng, [{} for _ in range(ng)]
    if not sweep:
        return np.zeros(G, np.int32), 1, [{}]
    keys = list(sweep)
    cols = [_per_game(sweep[k], G) for k in keys]
    table = np.concatenate(cols, axis=0).T                       # [G, sum rows]
    _, first, inv = np.unique(table, axis=0, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(first, kind="stable")                     # unique rows by first appearance
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    ids = rank[inv].astype(np.int32)
    values = []
    for u in order:
        g = int(first[u])
        d = {}
        for k, c in zip(keys, cols):
            d[k] = float(c[0, g]) if c.shape[0] == 1 else [float(x) for x in c[:, g]]
        values.append(d)
    return ids, len(values), values


# ---------------------------------------------------------------------------------------------- ranges, scales
def default_ranges(config):
    """[lo, hi] per quantity: rewards and total [0, a^2 / 4b] (the cartel value: with non-negative actions
    price * A_i <= (a - b A_i) A_i <= a^2 / 4b), action_i the agent's own action_range."""
    env = dict(_lib.ENV_DEFAULTS, **config["environment"])
    cartel = float(env["a"]) ** 2 / (4.0 * float(env["b"]))
    agents = config["agents"]
    out = [[0.0, cartel] for _ in agents]
    out += [[float(x) for x in a.get("action_range", _lib.QTABLE_DEFAULTS["action_range"])] for a in agents]
    out.append([0.0, cartel])
    return out


def resolve_ranges(config, override=None):
    """default_ranges with training.group_stats.ranges applied: keys are quantity names ("reward_0", "total"),
    or "reward" / "action" for every agent."""
    rng = default_ranges(config)
    names = quantity_names(len(config["agents"]))
    for k, v in (override or {}).items():
        lo, hi = float(v[0]), float(v[1])
        hit = [i for i, n in enumerate(names) if n == k or n.rsplit("_", 1)[0] == k]
        if not hit:
            raise ValueError("training.group_stats.ranges: unknown quantity %r (known: %s, reward, action)"
                             % (k, ", ".join(names)))
        for i in hit:
            rng[i] = [lo, hi]
    for n, (lo, hi) in zip(names, rng):
        if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
            raise ValueError("range of %s is [%r, %r): needs finite lo < hi" % (n, lo, hi))
    return rng


def fixed_scales(ranges, n_max):
    """[Q][2] powers of two: the largest s1, s2 with s1 * M * n_max <= 2^62 and s2 * M^2 * n_max <= 2^62,
    M = 16 * max(|lo|, |hi|) (include/thrl.h)."""
    n = float(max(1, int(n_max)))
    out = []
    for lo, hi in ranges:
        M = 16.0 * max(abs(lo), abs(hi))
        row = []
        for bound in (M * n, M * M * n):
            _, ex = math.frexp(bound)                 # bound <= 2^ex
            row.append(math.ldexp(1.0, 62 - ex))
        out.append(row)
    return out


# ---------------------------------------------------------------------------------------------- the spec
class GroupSpec:
    """Everything thrl_group_stats needs for one run's (or one shard's) local games.  ids: global group id of each
    local game; n_groups: the global count; n_max: largest group over the whole run (all shards), which sizes the
    fixed-point scales, so shards' sums add."""

    def __init__(self, n_agents, ids, n_groups, ranges, bins=DEFAULT_BINS, quantiles=DEFAULT_QUANTILES, n_max=None,
                 values=None, smooth=None):
        self.N = int(n_agents)
        self.Q = 2 * self.N + 1
        self.ids = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1))
        self.G = int(self.ids.size)
        self.n_groups = int(n_groups)
        if self.G < 1:
            raise ValueError("a group spec needs at least one game")
        if self.ids.min() < 0 or self.ids.max() >= self.n_groups:
            raise ValueError("group ids must lie in [0, %d)" % self.n_groups)
        self.counts = np.bincount(self.ids, minlength=self.n_groups).astype(np.int64)
        self.n_max = int(n_max) if n_max else int(self.counts.max())
        self.bins = int(bins)
        if not 1 <= self.bins <= _lib.STATS_MAX_BINS:
            raise ValueError("bins=%d out of [1, %d]" % (self.bins, _lib.STATS_MAX_BINS))
        self.quantiles = [float(q) for q in quantiles]
        self.ranges = [[float(lo), float(hi)] for lo, hi in ranges]
        if len(self.ranges) != self.Q:
            raise ValueError("%d ranges for Q=%d quantities" % (len(self.ranges), self.Q))
        self.lo = np.array([r[0] for r in self.ranges])
        self.hi = np.array([r[1] for r in self.ranges])
        self.inv_w = np.array([self.bins / (hi - lo) for lo, hi in self.ranges])
        self.scale = np.array(fixed_scales(self.ranges, self.n_max))
        self.perm = np.argsort(self.ids, kind="stable").astype(np.int32)
        self.seg_off = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.values = values if values is not None else [{} for _ in range(self.n_groups)]
        self.smooth = None if smooth is None else parse_halflife(smooth)       # the halflife, or None = off
        self._dev = {}

    @classmethod
    def from_config(cls, config, n_games, options=True, sweep=None, groups=None, n_groups=None):
        opt = parse_options(options)
        ids, ng, values = assign_groups(n_games, sweep=sweep, groups=groups, n_groups=n_groups)
        return cls(len(config["agents"]), ids, ng, resolve_ranges(config, opt["ranges"]), bins=opt["bins"],
                   quantiles=opt["quantiles"], n_max=opt["n_max"], values=values, smooth=opt.get("smooth"))

    def describe(self):
        """groups.json's content."""
        d = {"quantities": quantity_names(self.N), "bins": self.bins, "quantiles": self.quantiles,
             "ranges": self.ranges, "scales": self.scale.tolist(), "n_max": self.n_max,
             "groups": [{"id": k, "games": int(self.counts[k]), "values": self.values[k]}
                        for k in range(self.n_groups)]}
        if self.smooth is not None:
            d["smooth"] = {"halflife": self.smooth, "decay": ewm_decay(self.smooth)[1]}
        return d

    # ------------------------------------------------------------------ device
    def zeros(self, E, device):
        import torch
        shape = (int(E), self.n_groups, self.Q)
        return {"hist": torch.zeros(shape + (self.bins + 2,), dtype=torch.int32, device=device),
                "sums": torch.zeros(shape + (2,), dtype=torch.int64, device=device),
                "minmax": torch.zeros(shape + (2,), dtype=torch.int64, device=device)}

    def _device_index(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.perm).to(device), torch.from_numpy(self.seg_off).to(device))
        return self._dev[key]

    def reduce(self, L, rew, act, E, out, stream, at=0):
        """thrl_group_stats of device rows rew / act [>= E][N][G] (float64, contiguous) into rows at..at+E of `out`
        (self.zeros), on `stream` (a ctypes void pointer)."""
        if int(E) == 0:
            return out
        perm, seg = self._device_index(rew.device)
        a = _lib.GroupStatsArgs()
        a.n_games, a.n_agents, a.n_episodes, a.n_groups, a.n_bins = self.G, self.N, int(E), self.n_groups, self.bins
        a.game_reward_log, a.game_action_log = rew.data_ptr(), act.data_ptr()
        a.group_of = self.ids.ctypes.data_as(ctypes.c_void_p)
        a.perm, a.seg_off = perm.data_ptr(), seg.data_ptr()
        for q in range(self.Q):
            a.lo[q], a.hi[q], a.inv_w[q] = self.lo[q], self.hi[q], self.inv_w[q]
            a.scale[q][0], a.scale[q][1] = self.scale[q, 0], self.scale[q, 1]
        a.hist = out["hist"][at:].data_ptr()
        a.sums = out["sums"][at:].data_ptr()
        a.minmax = out["minmax"][at:].data_ptr()
        if rew.shape[1:] != (self.N, self.G) or act.shape[1:] != (self.N, self.G) or rew.shape[0] < E \
                or act.shape[0] < E or out["hist"].shape[0] < at + E:
            raise ThrlError("group stats: rows / outputs do not match the spec")
        _lib.check(L.thrl_group_stats(ctypes.byref(a), stream), "thrl_group_stats")
        return out


# ---------------------------------------------------------------------------------------------- smoothing
def ewm_decay(halflife):
    """(alpha, decay) of pandas' ewm(halflife=h): alpha = 1 - exp(log(0.5) / h) and decay = 1 - alpha, in double, in
    that order (include/thrl.h)."""
    alpha = 1.0 - math.exp(math.log(0.5) / float(halflife))
    return alpha, 1.0 - alpha


class Smoother:
    """The exponentially weighted mean of one run's (or one shard's) per-game rows, carried across launches
    (thrl_ewm_rows): state [2N][G] on the device (the numerators of reward_0..reward_{N-1}, action_0..action_{N-1}),
    den (the denominator, the same for every game) and rows (how many rows have gone through).  One Smoother lives
    as long as the curve it smooths; the result does not depend on how the rows are cut into apply() calls."""

    def __init__(self, n_agents, n_games, halflife, device):
        import torch
        self.N, self.G = int(n_agents), int(n_games)
        self.halflife = parse_halflife(halflife)
        self.alpha, self.decay = ewm_decay(self.halflife)
        self.state = torch.zeros((2 * self.N, self.G), dtype=torch.float64, device=device)
        self.den = 0.0
        self.rows = 0

    def apply(self, L, rew, act, E, stream, out=None):
        """Smooth rows 0..E of device rows rew / act [>= E][N][G] (float64, contiguous) in place, or into
        out = (reward_out, action_out) of the same layout, on `stream` (a ctypes void pointer).  Returns the two
        tensors that hold the smoothed rows."""
        o_r, o_a = (rew, act) if out is None else out
        if int(E) == 0:
            return o_r, o_a
        for t in (rew, act, o_r, o_a):
            if t.shape[1:] != (self.N, self.G) or t.shape[0] < E or str(t.dtype) != "torch.float64" \
                    or not t.is_contiguous() or t.device != self.state.device:
                raise ThrlError("smoother: rows must be contiguous float64 [>= %d][%d][%d] on %s"
                                % (E, self.N, self.G, self.state.device))
        a = _lib.EwmRowsArgs()
        a.n_games, a.n_agents, a.n_episodes = self.G, self.N, int(E)
        a.decay, a.den = self.decay, self.den
        a.reward_rows, a.action_rows = rew.data_ptr(), act.data_ptr()
        a.reward_out, a.action_out = o_r.data_ptr(), o_a.data_ptr()
        a.state_in = a.state_out = self.state.data_ptr()
        den = ctypes.c_double(self.den)
        a.den_out = ctypes.pointer(den)
        _lib.check(L.thrl_ewm_rows(ctypes.byref(a), stream), "thrl_ewm_rows")
        self.den = float(den.value)
        self.rows += int(E)
        return o_r, o_a


def ewm_host(rew, act, halflife, state=None, den=0.0):
    """numpy restatement of thrl_ewm_rows (the same float64 operations in the same order) of rows [E][N][G]:
    (smoothed rewards, smoothed actions, new state [2N][G], new den).  state / den: what an earlier call returned
    (None / 0 = fresh)."""
    rew = np.asarray(rew, np.float64)
    act = np.asarray(act, np.float64)
    E, N, G = rew.shape
    _, d = ewm_decay(halflife)
    num = np.zeros((2 * N, G)) if state is None else np.array(state, np.float64).reshape(2 * N, G)
    den = float(den)
    x = np.concatenate([rew, act], axis=1)                       # [E, 2N, G]
    y = np.empty_like(x)
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(E):
            num = x[e] + d * num                                # the product is rounded, then the sum
            den = 1.0 + d * den
            y[e] = num / den
    return y[:, :N], y[:, N:], num, den


def to_numpy(stats):
    """Device outputs (spec.zeros) as numpy: hist uint32, sums int64, minmax uint64."""
    return {"hist": stats["hist"].cpu().numpy().view(np.uint32), "sums": stats["sums"].cpu().numpy(),
            "minmax": stats["minmax"].cpu().numpy().view(np.uint64)}


# ---------------------------------------------------------------------------------------------- host side
def order_key(x):
    """The order-preserving uint64 image of float64 values (include/thrl.h)."""
    u = np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)
    neg = (u >> np.uint64(63)) != 0
    return np.where(neg, ~u, u | np.uint64(1 << 63))


def key_value(k):
    """Inverse of order_key."""
    k = np.asarray(k, np.uint64)
    pos = (k >> np.uint64(63)) != 0
    u = np.where(pos, k & ~np.uint64(1 << 63), ~k)
    return np.ascontiguousarray(u).view(np.float64)


def min_max(minmax):
    """(min, max) float64 from the stored keys; NaN where a cell holds no finite value."""
    mm = np.asarray(minmax).view(np.uint64) if np.asarray(minmax).dtype != np.uint64 else np.asarray(minmax)
    kmin, kmax = mm[..., 0], mm[..., 1]
    vmin = np.where(kmin == 0, np.nan, key_value(~kmin))
    vmax = np.where(kmax == 0, np.nan, key_value(kmax))
    return vmin, vmax


def merge(parts):
    """Exact combination of the outputs of disjoint sets of games (shards): hist and sums added, minmax max."""
    parts = list(parts)
    out = {"hist": np.array(parts[0]["hist"], dtype=np.uint32), "sums": np.array(parts[0]["sums"], dtype=np.int64),
           "minmax": np.array(parts[0]["minmax"]).view(np.uint64).copy()}
    for p in parts[1:]:
        out["hist"] += np.asarray(p["hist"], np.uint32)
        out["sums"] += np.asarray(p["sums"], np.int64)
        out["minmax"] = np.maximum(out["minmax"], np.asarray(p["minmax"]).view(np.uint64))
    return out


def moments(sums, hist, scale):
    """(mean, std) from the fixed-point sums; n = the cell's count in hist.  NaN for an empty cell."""
    n = np.asarray(hist, np.float64).sum(axis=-1)
    s = np.asarray(sums, np.int64)
    sc = np.asarray(scale, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = s[..., 0].astype(np.float64) / sc[:, 0] / n
        ex2 = s[..., 1].astype(np.float64) / sc[:, 1] / n
        std = np.sqrt(np.maximum(ex2 - mean * mean, 0.0))
    return mean, std


def quantiles(hist, vmin, vmax, qs, lo, hi):
    """The histogram quantiles of the module docstring: hist [..., Q, B+2], vmin / vmax [..., Q], lo / hi [Q]
    -> [..., Q, len(qs)]."""
    h = np.asarray(hist, np.int64)
    B = h.shape[-1] - 2
    lo = np.asarray(lo, np.float64)
    hi = np.asarray(hi, np.float64)
    w = (hi - lo) / B
    c = np.cumsum(h, axis=-1)
    n = c[..., -1].astype(np.float64)
    out = np.full(h.shape[:-1] + (len(qs),), np.nan)
    for j, q in enumerate(qs):
        t = q * n
        if q <= 0.0:
            out[..., j] = vmin
            continue
        if q >= 1.0:
            out[..., j] = vmax
            continue
        idx = np.sum(c < t[..., None], axis=-1)                  # first bin with cumulative count >= t
        idx = np.minimum(idx, B + 1)
        below = np.take_along_axis(c, np.maximum(idx - 1, 0)[..., None], -1)[..., 0].astype(np.float64)
        below = np.where(idx == 0, 0.0, below)
        inbin = np.take_along_axis(h, idx[..., None], -1)[..., 0].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            v = (lo + (idx - 1) * w) + (t - below) / inbin * w
        v = np.minimum(np.maximum(v, vmin), vmax)
        v = np.where(idx == 0, vmin, np.where(idx == B + 1, vmax, v))
        out[..., j] = np.where(n > 0, v, np.nan)
    return out


def finalize(raw, describe):
    """mean, std, min, max, quantiles (float64) from raw outputs (hist, sums, minmax) and a describe() dict."""
    vmin, vmax = min_max(raw["minmax"])
    mean, std = moments(raw["sums"], raw["hist"], describe["scales"])
    lo = [r[0] for r in describe["ranges"]]
    hi = [r[1] for r in describe["ranges"]]
    return {"mean": mean, "std": std, "min": vmin, "max": vmax,
            "quantiles": quantiles(raw["hist"], vmin, vmax, describe["quantiles"], lo, hi)}


def reduce_host(rew, act, ids, n_groups, describe):
    """numpy restatement of thrl_group_stats (same float64 operations): raw outputs of rows [E][N][G]."""
    rew = np.asarray(rew, np.float64)
    act = np.asarray(act, np.float64)
    E, N, G = rew.shape
    Q, B = 2 * N + 1, int(describe["bins"])
    ids = np.asarray(ids, np.int64)
    tot = rew[:, 0, :].copy()
    for i in range(1, N):
        tot = tot + rew[:, i, :]
    x = np.concatenate([rew, act, tot[:, None, :]], axis=1)     # [E, Q, G]
    lo = np.array([r[0] for r in describe["ranges"]])[None, :, None]
    hi = np.array([r[1] for r in describe["ranges"]])[None, :, None]
    inv_w = np.array([B / (h - l) for l, h in describe["ranges"]])[None, :, None]
    sc = np.asarray(describe["scales"], np.float64)
    M = 16.0 * np.maximum(np.abs(lo), np.abs(hi))
    fin = np.isfinite(x)
    with np.errstate(invalid="ignore"):
        b = np.floor((x - lo) * inv_w)
        b = 1 + np.minimum(np.where(np.isfinite(b), b, 0), B - 1).astype(np.int64)
        b = np.where(x < lo, 0, np.where(x >= hi, B + 1, b))
        b = np.where(fin, b, B + 1)
    xc = np.where(fin, np.minimum(np.maximum(x, -M), M), 0.0)
    v1 = np.rint(xc * sc[None, :, 0, None]).astype(np.int64)
    v2 = np.rint((xc * xc) * sc[None, :, 1, None]).astype(np.int64)
    k = order_key(np.where(fin, x, 0.0))
    ng = int(n_groups)
    cell = ((np.arange(E)[:, None, None] * ng + ids[None, None, :]) * Q + np.arange(Q)[None, :, None])  # [E, Q, G]
    hist = np.bincount((cell * (B + 2) + b).ravel(), minlength=E * ng * Q * (B + 2)).astype(np.uint32)
    hist = hist.reshape(E, ng, Q, B + 2)
    sums = np.zeros((E * ng * Q, 2), np.int64)
    np.add.at(sums[:, 0], cell.ravel(), v1.ravel())
    np.add.at(sums[:, 1], cell.ravel(), v2.ravel())
    mm = np.zeros((E * ng * Q, 2), np.uint64)
    np.maximum.at(mm[:, 0], cell.ravel(), np.where(fin, ~k, np.uint64(0)).ravel())
    np.maximum.at(mm[:, 1], cell.ravel(), np.where(fin, k, np.uint64(0)).ravel())
    sums, mm = sums.reshape(E, ng, Q, 2), mm.reshape(E, ng, Q, 2)
    return {"hist": hist, "sums": sums, "minmax": mm}


def save_json(path, describe):
    with open(path, "w") as f:
        json.dump(describe, f, indent=2)
