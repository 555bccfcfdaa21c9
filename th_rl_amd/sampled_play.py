"""Sampled play: the exact long-run profit of the STOCHASTIC policies the agents were trained with (thrl_price_probs,
thrl_sampled_chain, include/thrl.h), where every other analysis treats an agent as its greedy policy.

A Reinforce / ActorCritic agent learns a distribution (pi -> Categorical(...).sample()); a QTable agent plays
epsilon-greedily.  Without demand noise the price after a step is a function of the action tuple just played
(tuple_play.py), so under sampling the tuple played at a step is a Markov chain on the game's T tuples with
P(t -> t') = prod_i pi_i(a_i(t') | price(t)).  The row depends on t only through its price and many tuples share one, so
everything is indexed by the D <= T distinct prices of the config, and the row is a product over agents: a step costs
T D N multiplications and needs D sum_i A_i probabilities, never a T x T matrix.

tables(config) derives the per-config tables in numpy (tuple_play.tables' arrays, the distinct prices and the grouping of
the tuples by price); the device only reads them.  price_probs() evaluates the networks' softmax at a list of prices,
run() iterates the chain and returns per game (definitions in include/thrl.h) iters, change, mass, samp_price, agree [G],
samp_reward, samp_action [N, G], optionally pi [G, T].  `agree` is the long-run share of steps on which every agent plays
its greedy action.  summarize() gives per group converged, iters_*, delta_sampled_* (the profit gain of sampled play),
agree_mean and price_mean.  Sharded runs (th_rl_amd.launch) and CAC agents are out of scope.

Under demand noise (noise_prob > 0, NoisyPriceState) the next price is with probability p uniform on the tuple's band
of the price axis (tuple_stationary.py), where a network's probabilities live on a continuum: noise_tables(config,
resolution) gives the quadrature nodes (price 0, the atom of the clipped prices, and tuple_stationary's cell midpoints)
with their weights per tuple, and run(noise_prob=..., resolution=...) iterates thrl_sampled_noise_chain, which combines
both halves of the step; there start="reset" is the environment's reset distribution.  max_jump per game, the largest change
of a network's probability between adjacent nodes, says how honest the midpoint rule is.  With noise_prob = 0.0, the
default, everything here is the noise-free call as it was (and "reset" is no start of it); in train_one the noisy mode is
the sub-dict "noise" of training.sampled_play, so that every option dict valid before parses to what it did.
"""
import ctypes
import os

import numpy as np

from . import _lib
from . import analysis as an
from . import stationary as sn
from . import tuple_play as tp
from ._lib import ThrlError
from .deviation import optimal, profit_gain

DEFAULTS = dict(epsilon="current", start="uniform", tol=1e-12, max_iters=8192, pi=False)
NOISE_DEFAULTS = dict(noise_prob=None, resolution=1024)
STARTS = ("uniform", "state")
NOISE_STARTS = STARTS + ("reset",)
MAX_CELLS = _lib.STAT_MAX_CELLS
TILE = _lib.SPN_TILE
MAX_PRICES = _lib.STAT_MAX_CELLS
MAX_LDS = _lib.SP_MAX_LDS
GAME_FLOAT = ("change", "mass", "samp_price", "agree")
AGENT_FLOAT = ("samp_reward", "samp_action")
PER_GAME = ("iters", "start", "epsilon", "noise_prob", "max_jump") + GAME_FLOAT + AGENT_FLOAT + ("pi",)


def _check_eps(e, what):
    if isinstance(e, bool) or not isinstance(e, (int, float, np.integer, np.floating)) or not 0.0 <= float(e) <= 1.0:
        raise ValueError("%s must be a number in [0, 1], got %r" % (what, e))
    return float(e)


def parse_options(opt, config):
    """training.sampled_play (true or a dict) -> the dict with every key filled in: epsilon ("current": the QTable
    agents' epsilon where training stopped; a number, or one per agent), start ("uniform" or "state"), tol, max_iters,
    pi (store the distributions).  The optional key "response" (true or a dict, sampled_response.parse_options) asks for
    the best responses to the stochastic policies; it stays in the result, filled in, only when given, and together with
    "noise" it is refused unless it opts in with its own "noise": true (then the best responses are those under the same
    demand noise, at sampled_play's noise_prob and resolution).  The optional key "deviation" (true or a dict,
    sampled_deviation.parse_options) asks for the deviation test of sampled play; it stays in the result, filled in, only
    when given, and together with "noise" it is refused unless it opts in with its own "noise": true (then the test is the
    one under the same demand noise, at sampled_play's noise_prob and resolution).  The optional key "noise" (true or {"noise_prob": a number in [0, 1] or None = the
    run's own noise, refused for a noise-free run as training.greedy_stationary does; "resolution": the uniform cuts of
    the price axis behind the nodes}) asks for play under demand noise; it stays in the result, filled in, only when
    given, and with it start may be "reset".  Refuses a CAC agent, more than tuple_play.MAX_TUPLES tuples, more than
    MAX_CELLS - 1 cells and a working set above a CU's LDS."""
    name = "training.sampled_play"
    tp.check_config(config)
    noise = response = deviation = None
    if isinstance(opt, dict) and "deviation" in opt:
        opt = dict(opt)
        deviation = opt.pop("deviation")
        if deviation is None or deviation is False:
            deviation = None
    if isinstance(opt, dict) and "response" in opt:
        opt = dict(opt)
        response = opt.pop("response")
        if response is None or response is False:
            response = None
    if isinstance(opt, dict) and "noise" in opt:
        opt = dict(opt)
        noise = opt.pop("noise")
        if noise is None or noise is False:
            noise = None
        else:
            noise = an.options("sampled_play.noise", noise, NOISE_DEFAULTS)
    out = an.options("sampled_play", opt, DEFAULTS)
    e = out["epsilon"]
    if isinstance(e, (list, tuple)):
        if len(e) != len(config["agents"]):
            raise ValueError("%s.epsilon holds %d numbers, the game has %d agents" % (name, len(e), len(config["agents"])))
        out["epsilon"] = [_check_eps(x, name + ".epsilon") for x in e]
    elif e != "current":
        out["epsilon"] = _check_eps(e, name + ".epsilon")
    an.chain_options(out, name, STARTS if noise is None else NOISE_STARTS)
    ws = working_set(config)
    if not ws["fits"]:
        raise ValueError("%s: a game's working set is %d bytes (T=%d, D=%d), a CU's LDS holds %d"
                         % (name, ws["bytes"], ws["T"], ws["D"], MAX_LDS))
    if noise is not None:
        from . import tuple_stationary as ts
        if noise["noise_prob"] is None:
            an.check_own_noise(config, name + ".noise")
        else:
            noise["noise_prob"] = _check_eps(noise["noise_prob"], name + ".noise.noise_prob")
        noise["resolution"] = ts._check_resolution(noise["resolution"], name + ".noise.resolution")
        try:
            ws = working_set(config, resolution=noise["resolution"])
        except ValueError as e:
            raise ValueError("%s.noise: %s" % (name, e))
        if not ws["fits"]:
            raise ValueError("%s.noise: under noise a game's working set is %d bytes (T=%d, D=%d, Jn=%d), a CU's LDS holds %d"
                             % (name, ws["bytes"], ws["T"], ws["D"], ws["Jn"], MAX_LDS))
        out["noise"] = noise
    if response is not None:
        from . import sampled_response as sr
        opted = isinstance(response, dict) and response.get("noise") not in (None, False)     # (checked by its parser)
        if noise is not None and not opted:
            raise ValueError("%s: \"response\" with \"noise\": %s" % (name, sr.NOISE_FOLLOW_UP))
        out["response"] = sr.parse_options(response, config, noise=noise)
    if deviation is not None:
        from . import sampled_deviation as sd
        opted = isinstance(deviation, dict) and deviation.get("noise") not in (None, False)    # (checked by its parser)
        if noise is not None and not opted:
            raise ValueError("%s: \"deviation\" with \"noise\": %s" % (name, sd.NOISE_FOLLOW_UP))
        out["deviation"] = sd.parse_options(deviation, config, noise=noise)
    return out


def noisy(noise_prob):
    """True when thrl_sampled_noise_chain runs: any noise_prob (None, an array, a number) but the number 0.0."""
    plain = isinstance(noise_prob, (int, float, np.integer, np.floating)) and not isinstance(noise_prob, bool) \
        and float(noise_prob) == 0.0
    return not plain


# ---------------------------------------------------------------------------------------------- the per-config tables
def tables(config):
    """The per-config tables of thrl_sampled_chain (include/thrl.h) as a dict of numpy arrays: tuple_play.tables' T,
    n_actions, kinds, price [T], reward and scaled [N, T] as they are; dprice [D], the distinct values of price ascending
    (two prices are equal when their float64 bits are equal); row int32 [T], the index of price[t] in dprice; grp_first
    int32 [D + 1] and grp_perm int32 [T], the stable grouping of the tuples by row (ascending t inside a group);
    n_tuples, n_prices."""
    t = tp.tables(config)
    price = np.ascontiguousarray(t["price"], np.float64)
    # prices are >= +0.0, so the order of the bit patterns is the order of the values
    bits, row = np.unique(price.view(np.int64), return_inverse=True)
    row = row.reshape(-1).astype(np.int32)
    D = int(bits.size)
    perm = np.argsort(row, kind="stable").astype(np.int32)
    first = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=D))]).astype(np.int32)
    out = dict(t)
    out.update(dprice=np.ascontiguousarray(bits.view(np.float64)), row=row, grp_first=first, grp_perm=perm,
               n_tuples=int(t["T"]), n_prices=D)
    return out


def _r16(x):
    return (int(x) + 15) & ~15


def working_set(config, tabs=None, resolution=None, n_nodes=None):
    """The LDS bytes one game takes in thrl_sampled_chain, by include/thrl.h's formula: the sum of r16(x) over 8 T, 8 T
    (the iterates), 8 D, 8 D (W, Z), 4 D A_i per network, 2 D per QTable agent, 2 (D + 1), 2 T (the grouping),
    512 (2 N + 2) (staging) and 256 (constants).  Returns dict(bytes, T, D, fits): fits = within a CU's 160 KB.  With
    resolution (or n_nodes) the working set of thrl_sampled_noise_chain (spn_layout): beside that, r16(8 Jn) for V,
    r16(2 Jn) per QTable agent and two tile buffers of r16(4 (TILE A_i + 3)) per network; the dict also holds Jn.
    More than MAX_CELLS - 1 cells is a ValueError."""
    tabs = tables(config) if tabs is None else tabs
    T, D, N = int(tabs["n_tuples"]), int(tabs["n_prices"]), len(tabs["kinds"])
    b = 2 * _r16(8 * T) + 2 * _r16(8 * D)
    for kind, A in zip(tabs["kinds"], tabs["n_actions"]):
        b += _r16(2 * D) if kind == "QTable" else _r16(4 * D * int(A))
    b += _r16(2 * (D + 1)) + _r16(2 * T) + _r16(512 * (2 * N + 2)) + 256
    if resolution is None and n_nodes is None:
        return dict(bytes=int(b), T=T, D=D, fits=b <= MAX_LDS)
    Jn = int(n_nodes) if n_nodes is not None else n_nodes_of(config, resolution)
    b += _r16(8 * Jn)
    for kind, A in zip(tabs["kinds"], tabs["n_actions"]):
        b += _r16(2 * Jn) if kind == "QTable" else 2 * _r16(4 * (TILE * int(A) + 3))
    return dict(bytes=int(b), T=T, D=D, Jn=Jn, fits=b <= MAX_LDS)


def n_nodes_of(config, resolution):
    """Jn = the cells of tuple_stationary.cuts(config, resolution) plus the atom; ValueError above MAX_CELLS."""
    from . import tuple_stationary as ts
    J = int(ts.cuts(config, resolution).size - 1)
    if J + 1 > MAX_CELLS:
        raise ValueError("sampled_play: resolution=%d gives %d cells, at most %d (the atom of the clipped prices is one "
                         "more node)" % (resolution, J, MAX_CELLS - 1))
    return J + 1


def noise_tables(config, resolution=NOISE_DEFAULTS["resolution"], tabs=None):
    """The per-config tables of thrl_sampled_noise_chain (include/thrl.h): tables(config)'s arrays, and over the nodes
    xn [Jn] (0.0, the atom of the prices clipped to 0, then tuple_stationary's cell midpoints): node_w [Jn] (0, then
    cell_w), nn [T, Jn] (nn(t, 0) = z(t) / width, nn(t, 1 + k) = len_k(t) / width with tuple_stationary's len_k, z and
    width) as band_lo int32 [T] and band [T, W]; noise_price [T] and noise_reward [N, T] (tuple_stationary.tables');
    n_nodes, n_cells, band_w, resolution."""
    from . import tuple_stationary as ts
    out = dict(tables(config) if tabs is None else tabs)
    Jn = n_nodes_of(config, resolution)
    c = ts.cuts(config, resolution)
    geo = sn.noise_geometry(config, tp.tables(config), c)
    nn = np.concatenate([geo["z"][:, None], geo["length"]], axis=1) / geo["width"]
    band_lo, band = sn.band_of(nn)
    nprice = np.ascontiguousarray(geo["noise_price"])
    out.update(xn=np.concatenate([[0.0], geo["cell_x"]]), node_w=np.concatenate([[0.0], geo["cell_w"]]), nn=nn,
               band_lo=band_lo, band=band, noise_price=nprice,
               noise_reward=np.ascontiguousarray(nprice[None, :] * geo["quantity"]), cell_x=np.ascontiguousarray(geo["cell_x"]),
               cell_w=np.ascontiguousarray(geo["cell_w"]), n_nodes=Jn, n_cells=Jn - 1, band_w=int(band.shape[1]),
               resolution=int(resolution))
    return out


# ---------------------------------------------------------------------------------------------- the device calls
def _games(batch, n_games):
    G = an.games(batch, n_games, "sampled_play")
    if not getattr(batch, "initialized", True):
        raise ThrlError("sampled_play: call init_tables() or set_tables() first")
    return G


def price_probs(batch, prices, n_games=None):
    """thrl_price_probs: {agent index: device float32 [G, J, A_i]} for the Reinforce / ActorCritic agents of the first
    n_games (default all) games of `batch`: the softmax each samples from at the J prices `prices` (shared by the
    games), bit for bit what thrl_nn_act / thrl_ac_act return as prob_out.  An all-QTable batch gives {}.  Nothing of the
    batch is written."""
    import torch
    kinds = tp._kinds(batch)
    G = _games(batch, n_games)
    dev = batch.device
    with torch.cuda.device(dev):
        if isinstance(prices, torch.Tensor):
            x = prices.to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
        else:
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(prices, np.float64).reshape(-1))).to(dev)
        J = int(x.numel())
        if not 1 <= J <= MAX_PRICES:
            raise ThrlError("sampled_play: %d prices, the list must hold 1 to %d" % (J, MAX_PRICES))
        a = _lib.PriceProbsArgs()
        a.n_games, a.n_prices = G, J
        out = {}
        for i, k in enumerate(kinds):
            a.kind[i] = tp.KINDS[k]
            if k != "QTable" and k != "CAC":
                out[i] = torch.empty((G, J, int(batch.cfg.n_actions[i])), dtype=torch.float32, device=dev)
                a.nn_params[i] = batch.nn[i].params.data_ptr()
                a.prob[i] = out[i].data_ptr()
        a.price = x.data_ptr()
        _lib.check(batch.L.thrl_price_probs(ctypes.byref(batch.cfg), ctypes.byref(a), batch._stream()), "thrl_price_probs")
        torch.cuda.synchronize(dev)
    return out


def resolve_epsilon(batch, epsilon, G):
    """(eps [N] floats, eps_g device float64 [N, G] or None) for `epsilon`: "current" = the batch's epsilon now (the
    per-game sweep array where a sweep has one, else batch.eps); a number = every QTable agent's; N numbers; or an
    array [N, G] (device data: an entry outside [0, 1] refuses that game)."""
    import torch
    N = batch.N
    if isinstance(epsilon, str):
        if epsilon != "current":
            raise ThrlError("sampled_play: epsilon must be 'current', a number, N numbers or an array [N, G], got %r" % epsilon)
        sw = getattr(batch, "sweep", None) or {}
        if "eps" in sw:
            return [0.0] * N, sw["eps"][:, :G].to(torch.float64).contiguous()
        return [float(x) for x in list(batch.eps)[:N]], None
    if isinstance(epsilon, torch.Tensor) or np.ndim(epsilon) == 2:
        e = epsilon if isinstance(epsilon, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(epsilon, np.float64))
        e = e.to(device=batch.device, dtype=torch.float64)
        if e.dim() != 2 or e.shape[0] != N or e.shape[1] < G:
            raise ThrlError("sampled_play: a per-game epsilon must be [N=%d, G>=%d], got %s" % (N, G, tuple(e.shape)))
        return [0.0] * N, e[:, :G].contiguous()
    e = [float(epsilon)] * N if np.ndim(epsilon) == 0 else [float(x) for x in epsilon]
    if len(e) != N:
        raise ThrlError("sampled_play: epsilon holds %d numbers, the game has %d agents" % (len(e), N))
    kinds = tp._kinds(batch)
    for i, x in enumerate(e):
        if kinds[i] == "QTable" and not 0.0 <= x <= 1.0:
            raise ThrlError("sampled_play: epsilon[%d]=%r out of [0, 1]" % (i, x))
    return e, None


def resolve_noise(batch, noise_prob, G):
    """analysis.resolve_noise for run()'s noise_prob: a number lies in [0, 1]."""
    return an.resolve_noise(batch, noise_prob, G, "sampled_play", zero_ok=True)


def bind_rows(batch, kinds, G, who, *sets):
    """The networks' probability rows of a call: for each network i and each (what, rows, J, field) of `sets`, rows[i]
    must be a contiguous float32 tensor [G, J, A_i] on the batch's device, and field[i] takes its address.  who: the
    caller's name in the refusal."""
    import torch
    for i, k in enumerate(kinds):
        if k == "QTable":
            continue
        for what, rows, J, field in sets:
            x = rows.get(i)
            shape = (G, J, int(batch.cfg.n_actions[i]))
            if x is None or tuple(x.shape) != shape or x.dtype != torch.float32 or x.device != batch.state.device \
                    or not x.is_contiguous():
                raise ThrlError("%s: %s[%d] must be a contiguous float32 tensor %s on %s" % (who, what, i, shape, batch.device))
            field[i] = x.data_ptr()


def run(batch, epsilon="current", start="uniform", tol=1e-12, max_iters=8192, pi=False, n_games=None, tuple_policy=None,
        probs=None, dpolicy=None, tabs=None, noise_prob=0.0, resolution=NOISE_DEFAULTS["resolution"], nprobs=None, npolicy=None):
    """thrl_sampled_chain for the first n_games (default all) games of `batch` (a MixedGameBatch of QTable / Reinforce /
    ActorCritic agents, or a GameBatch).  epsilon: resolve_epsilon's rules.  start: "uniform" (1 / T on every tuple),
    "state" (the tuple whose price is the state the batch holds, tuple_play.start_tuples; a game whose state is no
    tuple's price is refused with iters = -1), or int [G] start tuples (outside [0, T): refused).  probs / dpolicy: the
    strategies at tabs["dprice"] ({i: float32 [G, D, A_i]} of price_probs, int16 [G, N, D] of
    tuple_stationary.price_policy; default: evaluated here; tuple_policy, tuple_play.extract()'s tensor, gives dpolicy
    without a device call, the tuple prices being the distinct prices repeated).

    noise_prob = 0.0 (the number) is that call and nothing else.  Otherwise thrl_sampled_noise_chain runs: noise_prob a
    number in (0, 1], an array [G] with entries in [0, 1] (zeros: the noise-free chain through the noisy call), or None
    (the batch's own: resolve_noise); start may then be "reset" = the tuple played at a uniform price on [0, a); resolution: the uniform cuts behind the nodes; tabs: noise_tables(batch.config,
    resolution); nprobs / npolicy: the strategies at tabs["xn"] ({i: float32 [G, Jn, A_i]} of price_probs, int16
    [G, N, Jn] of tuple_stationary.price_policy; default: evaluated here).  The result then also holds noise_prob and
    max_jump [G], n_nodes and resolution.  Returns a dict of numpy arrays."""
    import torch
    from . import tuple_stationary as ts
    N = batch.N
    G = _games(batch, n_games)
    given_start = not isinstance(start, str)
    noise = noisy(noise_prob)
    starts = NOISE_STARTS if noise else STARTS
    if not given_start and start not in starts:
        raise ThrlError("sampled_play: start must be one of %s or an array of tuples, got %r" % (starts, start))
    if isinstance(max_iters, bool) or not 1 <= int(max_iters) <= _lib.STAT_MAX_ITERS:
        raise ThrlError("sampled_play: max_iters=%r out of [1, %d]" % (max_iters, _lib.STAT_MAX_ITERS))
    if noise and (tabs is None or "xn" not in tabs):
        tabs = noise_tables(batch.config, resolution, tabs=tabs)
    if tabs is None:
        tabs = tables(batch.config)
    tp._batch_tables(batch, tabs)
    Jn, call = (int(tabs["n_nodes"]), "thrl_sampled_noise_chain") if noise else (None, "thrl_sampled_chain")
    ws = working_set(batch.config, tabs, n_nodes=Jn)
    if not ws["fits"]:                                   # what the call answers from the shape alone
        err = ThrlError("%s refused (thrl_err %d): %d bytes of LDS per game (T=%d, n_prices=%d%s), at most %d"
                        % (call, _lib.ERR_UNSUPPORTED, ws["bytes"], ws["T"], ws["D"], ", n_nodes=%d" % Jn if noise else "",
                           MAX_LDS))
        err.code = _lib.ERR_UNSUPPORTED
        raise err
    kinds = tp._kinds(batch)
    dev = batch.device
    sdev = batch.state.device
    T, D = int(tabs["n_tuples"]), int(tabs["n_prices"])
    a = _lib.SampledNoiseChainArgs() if noise else _lib.SampledChainArgs()
    a.n_games, a.n_tuples, a.n_prices, a.max_iters, a.tol = G, T, D, int(max_iters), float(tol)
    tab_list = [("grp_first", (D + 1,), np.int32), ("grp_perm", (T,), np.int32), ("reward", (N, T), np.float64),
                ("scaled", (N, T), np.float64), ("price", (T,), np.float64)]
    if noise:
        W = int(tabs["band_w"])
        a.n_nodes, a.band_w = Jn, W
        tab_list += [("band_lo", (T,), np.int32), ("band", (T, W), np.float64), ("noise_price", (T,), np.float64),
                     ("noise_reward", (N, T), np.float64), ("node_w", (Jn,), np.float64)]
    for i, k in enumerate(kinds):
        a.kind[i] = tp.KINDS[k]
    with torch.cuda.device(dev):
        eps, eps_g = resolve_epsilon(batch, epsilon, G)
        for i in range(N):
            a.eps[i] = eps[i]
        if eps_g is not None:
            a.eps_g = eps_g.data_ptr()
        if probs is None:
            probs = price_probs(batch, tabs["dprice"], n_games=G)
        if dpolicy is None:
            if tuple_policy is not None and an.is_policy(tuple_policy, (batch.G, N, T), sdev):
                rep = torch.from_numpy(np.asarray(tabs["grp_perm"])[np.asarray(tabs["grp_first"])[:-1]].astype(np.int64))
                dpolicy = tuple_policy[:G].index_select(2, rep.to(sdev)).contiguous()
            else:
                dpolicy = ts.price_policy(batch, tabs["dprice"], n_games=G)
        an.check_policy(batch, dpolicy, (G, N, D), "sampled_play", "dpolicy")
        bind_rows(batch, kinds, G, "sampled_play", ("probs", probs, D, a.prob))
        a.dpolicy = dpolicy.data_ptr()
        p_noise = p_g = None
        if noise:
            p_noise, p_g = resolve_noise(batch, noise_prob, G)
            if p_g is not None:
                a.noise_prob_g = p_g.data_ptr()
            else:
                a.noise_prob = p_noise
            if nprobs is None:
                nprobs = price_probs(batch, tabs["xn"], n_games=G)
            if npolicy is None:
                npolicy = ts.price_policy(batch, tabs["xn"], n_games=G)
            an.check_policy(batch, npolicy, (G, N, Jn), "sampled_play", "npolicy")
            bind_rows(batch, kinds, G, "sampled_play", ("nprobs", nprobs, Jn, a.nprob))
            a.npolicy = npolicy.data_ptr()
        keep = an.bind_tables(a, tabs, tab_list, dev, "sampled_play")
        t0 = None
        if given_start:
            t0 = an.start_tensor(start, G, dev, "sampled_play")
        elif start == "state":
            t0 = tp.start_tuples(batch.state[:G], tabs).to(torch.int32).contiguous()
        elif start == "reset":
            a.flags = _lib.SPN_START_RESET
        if t0 is not None:
            a.flags = _lib.SP_START_TUPLE                # THRL_SPN_START_TUPLE has the same value
            a.start = t0.data_ptr()
        out = an.outputs(dev, (("iters",), (G,), "int32"), (GAME_FLOAT, (G,), "float64"), (AGENT_FLOAT, (N, G), "float64"),
                         (("pi",) if pi else (), (G, T), "float64"), (("max_jump",) if noise else (), (G,), "float64"))
        an.bind(a, out)
        _lib.check(getattr(batch.L, call)(ctypes.byref(batch.cfg), ctypes.byref(a), batch._stream()), call)
        torch.cuda.synchronize(dev)
        res = an.fetch(out)
        res["epsilon"] = np.repeat(np.asarray(eps, np.float64)[:, None], G, axis=1) if eps_g is None else eps_g.cpu().numpy()
        if t0 is not None:
            res["start"] = t0.cpu().numpy()
        if noise:
            res["noise_prob"] = np.full(G, p_noise, np.float64) if p_g is None else p_g.cpu().numpy()
    res["T"], res["n_prices"], res["max_iters"], res["lds_bytes"] = T, D, int(max_iters), ws["bytes"]
    if noise:
        res["n_nodes"], res["resolution"] = Jn, int(tabs.get("resolution", resolution))
    return res


# ---------------------------------------------------------------------------------------------- host side
def summarize(games, ids, n_groups, nash, cartel, max_iters, cycle_reward=None, greedy_noise=None):
    """The summary rows, one per group: games, converged (solved and stopped before max_iters), iters_q25 / q50 / q75 /
    max, delta_sampled_mean / q25 / q50 / q75 (the profit gain of samp_reward, deviation.profit_gain), agree_mean,
    price_mean over the solved games.  cycle_reward [N, G] with lam [G] (the greedy cycles of the same run, where it has
    them): also delta_greedy_mean and randomness_cost_mean = delta_greedy - delta_sampled over the solved games that
    have a greedy cycle.  Games with max_jump (the noisy mode): also max_jump_max over the group's games, solved or not.
    greedy_noise (stat_reward [N, G], iters [G]: greedy play under the same noise, training.greedy_stationary of the
    same run): also delta_greedy_noise_mean and randomness_cost_noise_mean = delta_noise(greedy) - delta_sampled over the
    games solved by both."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    iters = np.asarray(games["iters"], np.int64)
    solved = iters >= 0
    delta = profit_gain(np.asarray(games["samp_reward"], np.float64), nash, cartel)
    price = np.asarray(games["samp_price"], np.float64)
    agree = np.asarray(games["agree"], np.float64)
    dgreedy = has = None
    if cycle_reward is not None:
        cr, lam = cycle_reward
        dgreedy = profit_gain(np.asarray(cr, np.float64), nash, cartel)
        has = np.asarray(lam).reshape(-1) > 0
    jump = np.asarray(games["max_jump"], np.float64) if "max_jump" in games else None
    dnoise = hasn = None
    if greedy_noise is not None:
        sr, git = greedy_noise
        dnoise = profit_gain(np.asarray(sr, np.float64), nash, cartel)
        hasn = np.asarray(git).reshape(-1) >= 0
    out = []
    for k in range(int(n_groups)):
        m = ids == k
        ms = m & solved
        row = {"group": k, "games": int(m.sum()),
               "converged": an.mean(solved[m] & (iters[m] < int(max_iters))) if m.any() else None}
        an.quantiles(row, "iters", iters[ms])
        row["iters_max"] = int(iters[ms].max()) if ms.any() else None
        row["delta_sampled_mean"] = an.mean(delta[ms])
        an.quantiles(row, "delta_sampled", delta[ms])
        row["agree_mean"] = an.mean(agree[ms])
        row["price_mean"] = an.mean(price[ms])
        if dgreedy is not None:
            mg = ms & has
            row["delta_greedy_mean"] = an.mean(dgreedy[mg])
            row["randomness_cost_mean"] = an.mean(dgreedy[mg] - delta[mg])
        if jump is not None:
            row["max_jump_max"] = an.num(jump[m].max()) if m.any() else None
        if dnoise is not None:
            mn = ms & hasn
            row["delta_greedy_noise_mean"] = an.mean(dnoise[mn])
            row["randomness_cost_noise_mean"] = an.mean(dnoise[mn] - delta[mn])
        out.append(row)
    return out


def combine(parts):
    """Per-game arrays of disjoint sets of games (in global game order) as one run's: concatenated along the game axis
    (axis 0 of pi [G, T], the last axis of the others)."""
    return an.combine(parts, other={"pi": 0}, only=PER_GAME)


def describe(options, T, n_prices, nash, cartel, summary, n_nodes=None):
    """sampled_play.json's content (n_nodes: the noisy mode's)."""
    d = {"options": options, "T": int(T), "n_prices": int(n_prices), "nash": nash, "cartel": cartel,
         "quantiles": list(sn.QUANTILES), "benchmark": "noise-free Nash and Cartel rewards (environment.get_optimal)",
         "summary": summary}
    if n_nodes is not None:
        d["n_nodes"] = int(n_nodes)
    return d


def save_games(d, r):
    """splay_iters int32 [G], splay_games float64 [4, G] (change, mass, samp_price, agree), splay_reward, splay_action and
    splay_epsilon float64 [N, G]; from start tuples splay_start int32 [G]; with the distributions splay_pi float64
    [G, T]; in the noisy mode splay_noise_prob and splay_max_jump float64 [G]."""
    np.save(os.path.join(d, "splay_iters.npy"), np.asarray(r["iters"], np.int32))
    np.save(os.path.join(d, "splay_games.npy"), np.stack([np.asarray(r[f], np.float64) for f in GAME_FLOAT]))
    np.save(os.path.join(d, "splay_reward.npy"), np.asarray(r["samp_reward"], np.float64))
    np.save(os.path.join(d, "splay_action.npy"), np.asarray(r["samp_action"], np.float64))
    np.save(os.path.join(d, "splay_epsilon.npy"), np.asarray(r["epsilon"], np.float64))
    for f, name in (("start", "splay_start.npy"), ("pi", "splay_pi.npy"), ("noise_prob", "splay_noise_prob.npy"),
                    ("max_jump", "splay_max_jump.npy")):
        path = os.path.join(d, name)
        if f in r:
            np.save(path, np.asarray(r[f], np.int32 if f == "start" else np.float64))
        elif os.path.isfile(path):               # a file left by an earlier run with other options
            os.remove(path)


def load_games(d):
    """The per-game arrays one run directory holds (training.sampled_play)."""
    gm = np.load(os.path.join(d, "splay_games.npy"))
    g = {"iters": np.load(os.path.join(d, "splay_iters.npy"))}
    g.update({f: gm[k] for k, f in enumerate(GAME_FLOAT)})
    g.update(samp_reward=np.load(os.path.join(d, "splay_reward.npy")), samp_action=np.load(os.path.join(d, "splay_action.npy")),
             epsilon=np.load(os.path.join(d, "splay_epsilon.npy")))
    for f, name in (("start", "splay_start.npy"), ("pi", "splay_pi.npy"), ("noise_prob", "splay_noise_prob.npy"),
                    ("max_jump", "splay_max_jump.npy")):
        if os.path.isfile(os.path.join(d, name)):
            g[f] = np.load(os.path.join(d, name))
    return g


def greedy_cycles_of(d, n_games):
    """(cycle_reward [N, G], lam [G]) of the self-play round of training.greedy_cycles in the same directory, or None
    when there is none or it holds another number of games."""
    pr, pc = os.path.join(d, "gcyc_cycle_reward.npy"), os.path.join(d, "gcyc_cycle.npy")
    if not (os.path.isfile(pr) and os.path.isfile(pc)):
        return None
    cr, cyc = np.load(pr), np.load(pc)
    if cr.ndim != 3 or cr.shape[2] != int(n_games) or cyc.shape[0] < 1:
        return None
    return cr[0], cyc[0, 1]


def greedy_noise_of(d, noise_prob):
    """(stat_reward [N, G], iters [G]) of training.greedy_stationary in the same directory when it analysed the same noise
    probabilities per game as noise_prob [G], else None."""
    if not os.path.isfile(os.path.join(d, "greedy_stationary.json")) or not os.path.isfile(os.path.join(d, "gstat_iters.npy")):
        return None
    from . import tuple_stationary as ts
    g = ts.load_games(d)
    p = np.asarray(noise_prob, np.float64).reshape(-1)
    if g["noise_prob"].shape != p.shape or not np.array_equal(g["noise_prob"], p):
        return None
    return g["stat_reward"], g["iters"]


def write_artefacts(exp_path, batch, config, opt, ids, n_groups, tuple_policy=None, with_cycles=False, spec=None,
                    histograms=False, budget=None):
    """train_one's training.sampled_play outputs: the per-game splay_*.npy files and sampled_play.json.  with_cycles:
    this run wrote the gcyc_* files (training.greedy_cycles) just before; only then does the summary carry
    delta_greedy_mean and randomness_cost_mean.  spec, histograms, budget: the run's group statistics, for the response
    curves of the sub-key "deviation"."""
    noise = opt.get("noise")
    tabs = noise_tables(config, noise["resolution"]) if noise else tables(config)
    noise_prob = 0.0
    if noise:       # a number goes per game, so that 0.0 too takes the noisy call and writes its files
        p = noise["noise_prob"]
        noise_prob = None if p is None else np.full(batch.G, float(p))
    r = run(batch, epsilon=opt["epsilon"], start=opt["start"], tol=opt["tol"], max_iters=opt["max_iters"], pi=opt["pi"],
            tuple_policy=tuple_policy, tabs=tabs, noise_prob=noise_prob)
    save_games(exp_path, r)
    nash, cartel = optimal(config)
    cyc = greedy_cycles_of(exp_path, np.asarray(r["iters"]).size) if with_cycles else None
    gn = greedy_noise_of(exp_path, r["noise_prob"]) if noise else None
    summary = summarize(r, ids, n_groups, nash, cartel, opt["max_iters"], cycle_reward=cyc, greedy_noise=gn)
    shown = {k: v for k, v in opt.items() if k not in ("response", "deviation")}    # their own files hold their options
    an.save_json(os.path.join(exp_path, "sampled_play.json"),
                 describe(shown, r["T"], r["n_prices"], nash, cartel, summary, n_nodes=r.get("n_nodes")))
    if opt.get("response"):
        from . import sampled_response as sr
        same = opt["pi"] and opt["start"] == "uniform"               # the stored distributions are the ones it would compute
        if opt["response"].get("noise"):
            sr.write_artefacts_noise(exp_path, batch, config, opt["response"], ids, n_groups, r["noise_prob"],
                                     epsilon=opt["epsilon"], tabs=tabs, pi=r["pi"] if same else None, max_jump=r["max_jump"])
        else:
            sr.write_artefacts(exp_path, batch, config, opt["response"], ids, n_groups, epsilon=opt["epsilon"], tabs=tabs,
                               pi=r["pi"] if same else None)
    if opt.get("deviation"):
        from . import sampled_deviation as sd
        same = opt["pi"] and opt["start"] == "uniform"
        more = dict(epsilon=opt["epsilon"], tabs=tabs, pi=r["pi"] if same else None, stat_iters=r["iters"] if same else None,
                    spec=spec, histograms=histograms, budget=budget)
        if opt["deviation"].get("noise"):
            sd.write_artefacts_noise(exp_path, batch, config, opt["deviation"], ids, n_groups, r["noise_prob"], **more)
        else:
            sd.write_artefacts(exp_path, batch, config, opt["deviation"], ids, n_groups, **more)
    return r
