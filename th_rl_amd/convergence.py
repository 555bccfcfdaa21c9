"""Convergence of trained QTable games (thrl_policy_track, include/thrl.h): the stopping rule of the
algorithmic-collusion literature (Calvano, Calzolari, Denicolo, Pastorello, AER 2020).  A game has converged when
no agent's greedy strategy -- the argmax of every row of its Q-table, first maximum -- has changed for W episodes.

The policy is compared at checks, every `every` episodes: a change that reverts between two checks is not seen, and
a game converges at the first check at episode e with e - stable_since >= W, where stable_since is the episode of
the last check that saw a change (or the baseline's).  Per game the device keeps:

    converged_at    episode of that first check, -1 = never (conv_episode.npy)
    conv_since      stable_since at that check, -1 = never (conv_since.npy)
    stable_since    episode of the last check that saw a change (conv_stable_since.npy); it goes on updating after
                    convergence, as does
    changes         the number of checks that saw a change (conv_changes.npy)

With snapshot=True the device also keeps each game's tables and state as they were at its convergence (one more
copy of the tables: stride * 4 B per game in float32, stride * 8 B in float64, plus 8 B of state; 16,976 B for the
headline config in float32), so the deviation analysis can run on the converged policy (training.deviation
"tables": "converged"; tables_at_convergence fills the slots of the games that never converged with their final
tables in place, so that analysis needs no third copy of the tables).

This module parses training.convergence, runs the kernel (Tracker) and summarises per group on the host:

    games, converged, fraction
    converged_at_mean / q25 / q50 / q75, conv_since_mean / q25 / q50 / q75   over the converged games
    still_stable    games whose policy has not changed for W episodes at the end of the run
                    (episode_end - stable_since >= W)
    changes_mean    mean number of checks that saw a change

Statistics that have no games are None.  Shards combine exactly: their per-game arrays are concatenated in global game
order (combine) and summarised as one run.
"""
import ctypes
import math
import os

import numpy as np

from . import _lib
from . import analysis as an
from ._lib import ThrlError
from .analysis import QUANTILES, save_json  # noqa: F401  (cv.save_json stays a public name)

DEFAULTS = dict(window=None, every=20, stop=None, snapshot=False)
PERIODS = 100000                # Calvano et al.: 100,000 periods without a change of any greedy strategy
FILES = {"converged_at": "conv_episode.npy", "conv_since": "conv_since.npy", "stable_since": "conv_stable_since.npy",
         "changes": "conv_changes.npy"}
NEURAL_FOLLOW_UP = ("convergence tracking runs on QTable agents only; neural agents (greedy = argmax pi) are a "
                    "follow-up on the mixed path's policy tables")


def check_config(config):
    """ValueError for a config with neural agents (the rule needs every agent's greedy table)."""
    an.check_qtable_only(config, "convergence", NEURAL_FOLLOW_UP)


def default_window(config):
    """ceil(100000 / max_steps) episodes: 100,000 periods."""
    T = int(dict(_lib.ENV_DEFAULTS, **config["environment"])["max_steps"])
    return int(math.ceil(PERIODS / T))


def parse_options(opt, config):
    """training.convergence (true or a dict) -> the dict with every key filled in: window W (episodes, default
    default_window), every (episodes between checks), stop (None or a fraction in (0, 1]), snapshot (bool)."""
    check_config(config)
    out = an.options("convergence", opt, DEFAULTS)
    if out["window"] is None:
        out["window"] = default_window(config)
    for k in ("window", "every"):
        v = out[k]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1:
            raise ValueError("training.convergence.%s must be an integer >= 1, got %r" % (k, v))
        out[k] = int(v)
    if out["stop"] is not None:
        s = out["stop"]
        if isinstance(s, bool) or not isinstance(s, (int, float)) or not 0 < float(s) <= 1:
            raise ValueError("training.convergence.stop must be null or a fraction in (0, 1], got %r" % (s,))
        out["stop"] = float(s)
    if not isinstance(out["snapshot"], bool):
        raise ValueError("training.convergence.snapshot must be true or false, got %r" % (out["snapshot"],))
    return out


def every_used(every, cycle=1):
    """`every` rounded up to a multiple of the training cycle (GameBatch: thrl_training_cycle), so that launches cut at
    the checks stay whole cycles of the wave kernel."""
    c = max(1, int(cycle))
    return -(-int(every) // c) * c


# ---------------------------------------------------------------------------------------------- the device side
class Tracker:
    """Convergence tracking of a GameBatch or an all-QTable MixedGameBatch: owns the device arrays, takes the
    baseline at batch.episode; check() runs thrl_policy_track at batch.episode."""

    def __init__(self, batch, window, every=1, snapshot=False):
        import torch
        if int(window) < 1 or int(every) < 1:
            raise ThrlError("Tracker: window and every must be >= 1, got %r, %r" % (window, every))
        if not batch.initialized:
            raise ThrlError("Tracker: call init_tables() or set_tables() on the batch first")
        self.batch, self.window, self.every, self.snapshot = batch, int(window), int(every), bool(snapshot)
        G = batch.G
        self.P = sum(int(batch.cfg.n_states[i]) + 1 for i in range(batch.N))
        dev = batch.device
        with torch.cuda.device(dev):
            self.policy = torch.zeros((G, self.P), dtype=torch.int16, device=dev)     # uint16 bits
            self.stable_since = torch.zeros((G,), dtype=torch.int64, device=dev)
            self.converged_at = torch.full((G,), -1, dtype=torch.int64, device=dev)
            self.conv_since = torch.full((G,), -1, dtype=torch.int64, device=dev)
            self.changes = torch.zeros((G,), dtype=torch.int32, device=dev)
            self.n_converged = torch.zeros((1,), dtype=torch.int32, device=dev)
            self.q_conv = torch.zeros_like(batch.q) if self.snapshot else None
            self.state_conv = torch.zeros((G,), dtype=torch.float64, device=dev) if self.snapshot else None
        self.last_check = int(batch.episode)
        self._launch(_lib.TRACK_BASELINE)

    def _launch(self, flags):
        import torch
        b = self.batch
        a = _lib.PolicyTrackArgs()
        a.n_games, a.flags, a.episode, a.window = b.G, int(flags), int(b.episode), self.window
        for f in ("policy", "stable_since", "converged_at", "conv_since", "changes", "n_converged"):
            setattr(a, f, getattr(self, f).data_ptr())
        a.state = b.state.data_ptr()
        if self.snapshot:
            a.q_conv, a.state_conv = self.q_conv.data_ptr(), self.state_conv.data_ptr()
        with torch.cuda.device(b.device):
            _lib.check(b.L.thrl_policy_track(ctypes.byref(b.cfg), b.q.data_ptr(), ctypes.byref(a), b._stream()),
                       "thrl_policy_track")

    def due(self):
        """True when batch.episode is a check episode (a multiple of `every`)."""
        return self.batch.episode % self.every == 0

    def check(self, count=True):
        """One check at batch.episode; returns the number of games converged so far (one small device-to-host copy,
        which waits for the device), or None with count=False (nothing waits)."""
        self._launch(0)
        self.last_check = int(self.batch.episode)
        return int(self.n_converged.item()) if count else None

    def converged(self):
        return int(self.n_converged.item())

    def to_numpy(self):
        """Per-game arrays: converged_at, conv_since, stable_since (int64 [G]), changes (int32 [G]), policy (uint16
        [G, P]); with snapshot q_conv [G, stride] and state_conv [G]."""
        out = {f: getattr(self, f).cpu().numpy() for f in FILES}
        out["policy"] = self.policy.cpu().numpy().view(np.uint16)
        if self.snapshot:
            out["q_conv"], out["state_conv"] = self.q_conv.cpu().numpy(), self.state_conv.cpu().numpy()
        return out

    def state_dict(self):
        sd = dict(version=1, window=self.window, every=self.every, snapshot=self.snapshot, last_check=self.last_check,
                  n_games=int(self.batch.G), P=self.P)
        for f in ("policy", "stable_since", "converged_at", "conv_since", "changes", "n_converged"):
            sd[f] = getattr(self, f).cpu()
        if self.snapshot:
            sd["q_conv"], sd["state_conv"] = self.q_conv.cpu(), self.state_conv.cpu()
        return sd

    def load_state_dict(self, sd):
        if int(sd["n_games"]) != self.batch.G or int(sd["P"]) != self.P or int(sd["window"]) != self.window:
            raise ThrlError("convergence state does not match this tracker (games / policy size / window)")
        if bool(sd["snapshot"]) and not self.snapshot:
            raise ThrlError("convergence state has a snapshot; this tracker keeps none")
        for f in ("policy", "stable_since", "converged_at", "conv_since", "changes", "n_converged"):
            getattr(self, f).copy_(sd[f])
        if self.snapshot:
            if not bool(sd["snapshot"]):
                raise ThrlError("convergence state has no snapshot; this tracker keeps one")
            self.q_conv.copy_(sd["q_conv"])
            self.state_conv.copy_(sd["state_conv"])
        self.last_check = int(sd["last_check"])
        return self

    def save(self, path):
        import torch
        torch.save(self.state_dict(), path)

    def load(self, path):
        import torch
        return self.load_state_dict(torch.load(path, weights_only=True))

    def tables_at_convergence(self, chunk=65536):
        """(q [G, stride], state [G]) on the device: each converged game's snapshot, the current tables and state of
        the others.  Built in place in the snapshot: the slots of the games not converged (which the kernel writes
        only when a game converges) take the batch's tables and state, `chunk` games at a time, so the only extra
        device memory is one chunk's rows.  Later checks are unaffected; state_dict() then carries the filled slots."""
        import torch
        if not self.snapshot:
            raise ThrlError("Tracker: tables at convergence need snapshot=True")
        for lo in range(0, self.batch.G, int(chunk)):
            hi = min(lo + int(chunk), self.batch.G)
            m = self.converged_at[lo:hi] < 0
            self.q_conv[lo:hi][m] = self.batch.q[lo:hi][m]
            self.state_conv[lo:hi][m] = self.batch.state[lo:hi][m]
        torch.cuda.synchronize(self.batch.device)
        return self.q_conv, self.state_conv


# ---------------------------------------------------------------------------------------------- host side
def _stats(x, prefix):
    out = {prefix + "_mean": an.mean(x)}
    an.quantiles(out, prefix, x)
    return out


def summarize(games, ids, n_groups, window, episode_end):
    """One dict per group: games = dict of per-game arrays (FILES' fields) in global game order, ids = group id per
    game, episode_end = the global episode the run ended at."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    ca = np.asarray(games["converged_at"], np.int64)
    cs = np.asarray(games["conv_since"], np.int64)
    ss = np.asarray(games["stable_since"], np.int64)
    ch = np.asarray(games["changes"], np.int64)
    out = []
    for k in range(int(n_groups)):
        m = ids == k
        n = int(m.sum())
        c = m & (ca >= 0)
        r = {"group": k, "games": n, "converged": int(c.sum()), "fraction": an.num(c.sum() / n) if n else None}
        r.update(_stats(ca[c].astype(np.float64), "converged_at"))
        r.update(_stats(cs[c].astype(np.float64), "conv_since"))
        r["still_stable"] = int(np.sum(m & (int(episode_end) - ss >= int(window))))
        r["changes_mean"] = an.num(ch[m].mean()) if n else None
        out.append(r)
    return out


def combine(parts):
    """Per-game arrays of disjoint shards (in global game order) as one run's: concatenated along the game axis."""
    return an.combine(parts)


def describe(options, every, episodes_run, episode_end, stopped_early, summary):
    """convergence.json's content."""
    return {"options": options, "every_used": int(every), "episodes_run": int(episodes_run),
            "episode_end": int(episode_end), "stopped_early": bool(stopped_early), "quantiles": list(QUANTILES),
            "summary": summary}


def load_games(d):
    """The per-game arrays one run directory (or shard) holds."""
    return {f: np.load(os.path.join(d, name)) for f, name in FILES.items()}


def save_games(d, games):
    for f, name in FILES.items():
        np.save(os.path.join(d, name), np.asarray(games[f], np.int32 if f == "changes" else np.int64))


def truncate_rows(path, rows):
    """Rewrite the .npy at `path` with its first `rows` rows (the per-epoch artefacts of a run that stopped early)."""
    a = np.load(path, mmap_mode="r")
    if a.shape[0] == rows:
        return
    head = np.array(a[:rows])
    del a
    tmp = path + ".tmp.npy"
    np.save(tmp, head)
    os.replace(tmp, path)


def merged(shards, out, config, opt, ids, n_groups, first):
    """convergence.json and conv_*.npy of a sharded run (launch.merge_analysis); what only a run knows (every_used,
    episodes_run, episode_end, stopped_early) is shard 0's: every rank stops at the same episode."""
    games = combine(load_games(s) for s in shards)
    save_games(out, games)
    summary = summarize(games, ids, n_groups, opt["window"], first["episode_end"])
    return describe(opt, first["every_used"], first["episodes_run"], first["episode_end"], first["stopped_early"], summary)


def write_artefacts(exp_path, batch, config, opt, ids, n_groups, tracker, every, episodes_run, stopped_early):
    """train_one's training.convergence outputs: the conv_*.npy per-game arrays, convergence.json and convergence.pt."""
    games = tracker.to_numpy()
    save_games(exp_path, games)
    end = int(tracker.batch.episode)
    summary = summarize(games, ids, n_groups, opt["window"], end)
    save_json(os.path.join(exp_path, "convergence.json"),
              describe(opt, every, episodes_run, end, stopped_early, summary))
    tracker.save(os.path.join(exp_path, "convergence.pt"))
