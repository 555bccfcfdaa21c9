"""Every refusal of the analysis entry points keeps its return code and its words.

tests/golden/api_refusals.json holds (entry point, case, return code, thrl_last_error()) for every case below, recorded
from the library before the analysis wrappers were split off into thrl_api_analysis.hip and their repeated checks
became shared helpers.  The test replays the cases and compares; it never writes the file (that is
`python tests/test_api_refusals_host.py --record`).  The bad-argument tables are the ones the *_host.py tests of the
individual analyses already have.  The entries of thrl_sampled_response, thrl_sampled_response_noise, thrl_sampled_deviation
and thrl_sampled_deviation_noise were added later, from the library before the deviation pair's checks became sd_check_args
and sd_copy_common; the entries that were there came out of that recording byte for byte.

The module also runs where a GPU is present, so no case may get as far as a launch even if its refusal were lost: every
args struct leaves NULL a pointer that the entry point's last NULL check tests (LAST_NULL, asserted before every call),
so the worst a mistake can do is THRL_ERR_NULL and a failing comparison.  No GPU is needed.

The two episode entry points are here for one refusal each: parity mode with a QTable agent of more than 128 actions, whose
choices the injected int8 format cannot hold.  Behind it thrl_qtable_episodes finds no replay memory and
thrl_mixed_episodes no kernel for more than 64 actions, so these cases cannot launch either."""
import ctypes
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import test_attractors_host as AT
import test_convergence_host as CV
import test_crossplay_host as XP
import test_deviation_host as DV
import test_equilibrium_host as EQ
import test_sampled_deviation_host as SD
import test_sampled_deviation_noise_host as SDN
import test_sampled_host as SC
import test_sampled_noise_host as SN
import test_sampled_response_host as SR
import test_sampled_response_noise_host as SRN
import test_stationary_host as ST
import test_tuple_analysis_host as TA
import test_tuple_attractors_host as TT
import test_tuple_play_host as TP
import test_tuple_stationary_host as TS

GOLDEN = os.path.join(ROOT, "tests", "golden", "api_refusals.json")
CSRC = os.path.join(ROOT, "th_rl_amd", "csrc")
FAKE = 4096                           # never dereferenced: every case is refused before any launch
AG = dict(name="QTable", gamma=0.95, actions=21, states=100, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)


def _two(a0=21, a1=21, **second):
    return {"agents": [dict(AG, actions=a0), dict(AG, actions=a1, **second)], "environment": dict(ENV)}


CONFIGS = {
    "base": _two(),
    "forty": _two(21, 40),            # a network has at most 32 actions
    "wide": _two(129, 32),            # 4,128 tuples in tuple form
    "eq_wide": _two(65, 64),          # 4,160 tuples for the plan of thrl_equilibrium
    "eq_fine": {"agents": [dict(AG, actions=64, states=30000), dict(AG, actions=64, states=30000, action_range=[0.2, 0.4037])],
                "environment": dict(ENV)},      # more than 1,024 distinct row tuples
    "gamma_one": _two(gamma=1.0),
    "gamma_nan": _two(gamma=float("nan")),
    "sp_big": _two(32, 32),           # thrl_sampled_chain's working set does not fit
    "sr_big": _two(26, 32),           # the lightest shapes whose working sets the four newer calls on sampled play refuse
    "srn_big": _two(35, 21),
    "sd_big": _two(35, 32),
    "sdn_big": _two(35, 28),
    "inj_wide": _two(129, 21),        # one action more than an injected int8 choice holds
    "inj_wide_second": _two(21, 129),
}


def _bad(test_fn):
    """The parametrize list of an existing test."""
    return list(test_fn.pytestmark[0].args[1])


def _ident(kw):
    return ",".join("%s=%r" % (k, v) for k, v in kw.items()) or "baseline"


def _set(v):
    return bool(v)                    # a c_void_p field reads back None when NULL


def _neural(a, fields):
    return [getattr(a, f)[i] for i in range(2) if a.kind[i] != 0 for f in fields]


# The pointers the entry point's last NULL check tests, under the case's own flags and kinds.  (thrl_tuple_policy and
# thrl_price_policy end in "q is NULL with a QTable agent": every case here has one.)
LAST_NULL = {
    "thrl_group_stats": lambda a, q: [a.game_reward_log, a.game_action_log, a.group_of, a.perm, a.seg_off, a.hist, a.sums, a.minmax],
    "thrl_deviation": lambda a, q: [q] + [getattr(a, f) for f in ("state0", "mu", "lam", "mu_post", "lam_post", "ret_step",
                                                                   "act_dev", "cycle_reward", "cycle_action", "gain")],
    "thrl_policy_track": lambda a, q: [q] + [getattr(a, f) for f in ("policy", "stable_since", "converged_at", "conv_since", "changes")],
    "thrl_crossplay": lambda a, q: [getattr(a, f) for f in XP.FIELDS] if a.flags & 1 else [q],
    "thrl_tuple_policy": lambda a, q: [q],
    "thrl_price_policy": lambda a, q: [q],
    "thrl_tuple_walk": lambda a, q: [getattr(a, f) for f in TP.WALK_FIELDS],
    "thrl_tuple_deviation": lambda a, q: [getattr(a, f) for f in TA.DEV_FIELDS],
    "thrl_tuple_equilibrium": lambda a, q: [getattr(a, f) for f in TA.EQ_FIELDS],
    "thrl_tuple_attractors": lambda a, q: [getattr(a, f) for f in (TT.WEIGHTED if a.start_w else TT.REQUIRED)],
    "thrl_tuple_stationary": lambda a, q: [a.start] if a.flags & 1 else [getattr(a, f) for f in TS.TS_REQUIRED[-6:]],
    "thrl_price_probs": lambda a, q: _neural(a, ("nn_params", "prob")),
    "thrl_sampled_chain": lambda a, q: [a.start] if a.flags & 1 else [getattr(a, f) for f in SC.SC_REQUIRED[-7:]],
    "thrl_sampled_noise_chain": lambda a, q: [a.start] if a.flags & 1 else [getattr(a, f) for f in SN.SN_REQUIRED[-7:]],
    "thrl_sampled_response": lambda a, q: [getattr(a, f) for f in (SR.SR_WEIGHTED if a.pi else SR.SR_REQUIRED[-5:])],
    "thrl_sampled_response_noise": lambda a, q: [getattr(a, f) for f in (SRN.SRN_WEIGHTED if a.pi else SRN.SRN_OUTPUTS)],
    "thrl_sampled_deviation": lambda a, q: [getattr(a, f) for f in SD.SD_OUTPUTS],
    "thrl_sampled_deviation_noise": lambda a, q: [getattr(a, f) for f in SDN.SDN_OUTPUTS],
    "thrl_equilibrium": lambda a, q: [q] + [getattr(a, f) for f in ("state0", "mu", "lam", "iters", "n_diff_all", "n_diff_on",
                                                                     "loss_all", "loss_on", "loss_all_mean", "loss_on_mean", "v_on")],
    "thrl_attractors": lambda a, q: ([q] if not a.flags & 1 else [getattr(a, f) for f in AT.RESET] if a.n_starts > 0
                                     else [getattr(a, f) for f in ("state0", "policy") + AT.OUTPUTS]),
    "thrl_stationary": lambda a, q: ([q] if not a.flags & 1 else [a.state0] if a.flags & 2
                                     else [getattr(a, f) for f in ("policy",) + ST.OUTPUTS]),
    # (what is left unset behind the refusal under test: see the module docstring)
    "thrl_qtable_episodes": lambda a, q: [a.replay_mem],
    "thrl_mixed_episodes": lambda a, q: [a.policy_tab],
}
TAKES_Q = {"thrl_deviation", "thrl_policy_track", "thrl_crossplay", "thrl_tuple_policy", "thrl_price_policy", "thrl_equilibrium",
           "thrl_attractors", "thrl_stationary"}


def _gs_args(**kw):
    from th_rl_amd import _lib
    a = _lib.GroupStatsArgs()
    a.n_games, a.n_agents, a.n_episodes, a.n_groups, a.n_bins = 64, 2, 10, 3, 256
    for f in ("game_reward_log", "game_action_log", "group_of", "perm", "seg_off", "hist", "sums"):
        setattr(a, f, FAKE)           # minmax stays NULL: the one NULL check is the last refusal any case can reach
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _tuple_policy(**kw):
    kinds = kw.pop("kinds", (0, 1))
    return TP._policy_args(kinds=kinds, **kw)


def _episode_buffers(**kw):
    from th_rl_amd import _lib
    b = _lib.Buffers()
    for f in ("q", "state", "inj_u", "inj_choice"):
        setattr(b, f, FAKE)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _mixed_args(kind=(0, 0), **kw):
    from th_rl_amd import _lib
    mx = _lib.Mixed()
    for i, k in enumerate(kind):
        mx.kind[i] = k
        if k:
            mx.nn_params[i] = FAKE
    for f in ("inj_u", "inj_choice", "inj_action"):
        setattr(mx, f, FAKE)
    for k, v in kw.items():
        setattr(mx, k, v)
    return mx


def cases():
    """[(entry point, case id, config name or None, q, args or None)]; q is ignored by entry points that take none."""
    out, seen = [], set()

    def add(entry, build, kw, cfg="base", q=FAKE, ident=None):
        ident = ident or _ident(dict(kw, **({"cfg": cfg} if cfg != "base" else {})))
        if (entry, ident) not in seen:          # (the tables of two tests may share a case)
            seen.add((entry, ident))
            out.append((entry, ident, cfg, q, build(**kw)))

    def nulls(entry, build, base_kw=None, q=FAKE):
        out.append((entry, "args=NULL", "base", q, None))
        out.append((entry, "cfg=NULL", None, q, build(**(base_kw or {}))))

    # counts and kinds of a game in tuple form, through every entry point that checks them
    def tuple_counts(entry, build, g, extra=None, q=FAKE):
        for n in (0, 440, 4097):
            add(entry, build, dict(g, n_tuples=n, **(extra or {})), q=q)
        add(entry, build, dict(g, n_tuples=4128, **(extra or {})), cfg="wide", q=q)

    def tuple_kinds(entry, build, g, forty_kw):
        for k in ([0, 3], [0, 4], [-1, 0]):
            add(entry, build, dict(g, kind=k))
        add(entry, build, dict(g, kind=[0, 1], **forty_kw), cfg="forty")

    # ---- thrl_group_stats (its checks past the NULL check need every pointer set: see UNREACHED)
    for kw in (dict(n_games=0), dict(n_agents=0), dict(n_agents=9), dict(n_episodes=-1), dict(n_groups=0), dict(n_bins=0),
               dict(n_bins=1025), dict(reserved=1), dict()):
        out.append(("thrl_group_stats", _ident(kw), None, None, _gs_args(**kw)))
    for f in ("game_reward_log", "group_of", "hist"):
        out.append(("thrl_group_stats", "%s=None" % f, None, None, _gs_args(**{f: None, "minmax": FAKE})))
    out.append(("thrl_group_stats", "args=NULL", None, None, None))

    # ---- thrl_deviation
    g = dict(gain=None)
    for kw in _bad(DV.test_bad_arguments_are_bad_config):
        add("thrl_deviation", DV._args, dict(g, **kw))
    for f in _bad(DV.test_missing_outputs_are_null):
        if f not in ("q", "args"):
            add("thrl_deviation", DV._args, dict(g, **{f: None}))
    add("thrl_deviation", DV._args, {}, q=None, ident="q=None")
    nulls("thrl_deviation", DV._args, g)

    # ---- thrl_policy_track
    g = dict(changes=None)
    for kw in _bad(CV.test_bad_arguments_are_bad_config):
        add("thrl_policy_track", CV._args, dict(g, **kw))
    for f in ("policy", "stable_since", "converged_at", "conv_since", "changes"):
        add("thrl_policy_track", CV._args, dict(g, **{f: None}))
    add("thrl_policy_track", CV._args, {}, q=None, ident="q=None")
    nulls("thrl_policy_track", CV._args, g)

    # ---- thrl_crossplay (without the flag q is the last pointer tested; with it, the arrays are)
    for kw in _bad(XP.test_bad_arguments_are_bad_config):
        add("thrl_crossplay", XP._args, dict(kw, cycle_action=None), q=None)
    for f in XP.FIELDS:
        add("thrl_crossplay", XP._args, {f: None}, q=None)
    add("thrl_crossplay", XP._args, {}, q=None, ident="q=None")
    add("thrl_crossplay", XP._args, dict(flags=1, policy=None), q=None)
    nulls("thrl_crossplay", XP._args, q=None)

    # ---- thrl_tuple_policy, thrl_price_policy (q = NULL with a QTable agent is their last refusal)
    for kw in (dict(n_games=0), dict(n_games=65), dict(n_tuples=21), dict(price=None), dict(tuple_policy=None), dict()):
        add("thrl_tuple_policy", _tuple_policy, kw, q=None)
    tuple_counts("thrl_tuple_policy", _tuple_policy, {}, q=None)
    for k in ((0, 3), (0, 4), (-1, 0)):
        add("thrl_tuple_policy", _tuple_policy, dict(kinds=k), q=None)
    add("thrl_tuple_policy", _tuple_policy, dict(n_tuples=21 * 40), cfg="forty", q=None)
    a = _tuple_policy()
    a.nn_params[1] = None
    out.append(("thrl_tuple_policy", "nn_params[1]=None", "base", None, a))
    nulls("thrl_tuple_policy", _tuple_policy, q=None)
    for kw in TS.PP_BAD + [dict(kind=[3, 0]), dict(n_prices=4097), dict(price=None), dict(price_policy=None), dict(kind=[0, 2]), dict()]:
        add("thrl_price_policy", TS.pp_args, kw, cfg="forty" if kw.get("kind") == [0, 1] else "base", q=None)
    nulls("thrl_price_policy", TS.pp_args, q=None)

    # ---- thrl_tuple_walk, thrl_tuple_deviation, thrl_tuple_equilibrium, thrl_tuple_attractors
    g = dict(cycle_action=None)
    for kw in _bad(TP.test_tuple_walk_bad_arguments_are_bad_config):
        add("thrl_tuple_walk", TP._walk_args, dict(g, **kw))
    tuple_counts("thrl_tuple_walk", TP._walk_args, g)
    for f in TP.WALK_FIELDS:
        add("thrl_tuple_walk", TP._walk_args, dict(g, **{f: None}))
    nulls("thrl_tuple_walk", TP._walk_args, g)
    g = dict(gain=None)
    for kw in _bad(TA.test_tuple_deviation_bad_arguments_are_bad_config):
        add("thrl_tuple_deviation", TA._dev_args, dict(g, **kw))
    tuple_counts("thrl_tuple_deviation", TA._dev_args, g)
    for f in TA.DEV_FIELDS:
        add("thrl_tuple_deviation", TA._dev_args, dict(g, **{f: None}))
    nulls("thrl_tuple_deviation", TA._dev_args, g)
    g = dict(v_on=None)
    for kw in _bad(TA.test_tuple_equilibrium_bad_arguments_are_bad_config) + [dict(agents=-1)]:
        add("thrl_tuple_equilibrium", TA._eq_args, dict(g, **kw))
    tuple_counts("thrl_tuple_equilibrium", TA._eq_args, g)
    for kw, cfg in ((dict(), "gamma_one"), (dict(agents=2), "gamma_nan"), (dict(agents=1), "gamma_one"),
                    (dict(sweep_gamma=FAKE), "gamma_one")):
        add("thrl_tuple_equilibrium", TA._eq_args, dict(g, **kw), cfg=cfg)
    for f in TA.EQ_FIELDS:
        add("thrl_tuple_equilibrium", TA._eq_args, dict(g, **{f: None}))
    nulls("thrl_tuple_equilibrium", TA._eq_args, g)
    g = dict(slot_x0=None)
    for kw in _bad(TT.test_bad_arguments_are_bad_config):
        add("thrl_tuple_attractors", TT._args, dict(g, **kw))
    tuple_counts("thrl_tuple_attractors", TT._args, g)
    for f in TT.REQUIRED:
        add("thrl_tuple_attractors", TT._args, dict(g, **{f: None}))
    for f in TT.WEIGHTED:
        add("thrl_tuple_attractors", TT._args, dict({w: FAKE for w in TT.WEIGHTED}, start_w=FAKE, **{f: None}))
    nulls("thrl_tuple_attractors", TT._args, g)

    # ---- thrl_tuple_stationary
    g = dict(stat_price=None)
    for kw in TS.TS_BAD + [dict(n_cells=4097), dict(noise_prob=0.0, noise_prob_g=FAKE)]:
        add("thrl_tuple_stationary", TS.ts_args, dict(g, **kw), cfg="forty" if kw.get("n_tuples") == 21 * 40 else "base")
    tuple_counts("thrl_tuple_stationary", TS.ts_args, g)
    tuple_kinds("thrl_tuple_stationary", TS.ts_args, g, dict(n_tuples=21 * 40))
    for f in TS.TS_REQUIRED:
        add("thrl_tuple_stationary", TS.ts_args, dict(g, **{f: None}))
    add("thrl_tuple_stationary", TS.ts_args, dict(flags=1))
    nulls("thrl_tuple_stationary", TS.ts_args, g)

    # ---- thrl_price_probs (agent 1 is a network in every case: its prob is the pointer left NULL)
    g = dict(prob=[None, None])
    for kw in SC.PB_BAD:
        kw = dict(kw)
        cfg = "forty" if kw.pop("forty", False) else "base"
        add("thrl_price_probs", SC.pb_args, dict(g, **kw), cfg=cfg)
    for kw in (dict(kind=[3, 1]), dict(n_prices=4097), dict(price=None), dict(nn_params=[None, None]), dict()):
        add("thrl_price_probs", SC.pb_args, dict(g, **kw))
    nulls("thrl_price_probs", SC.pb_args, g)

    # ---- thrl_sampled_chain, thrl_sampled_noise_chain
    g = dict(agree=None)
    for kw in SC.SC_BAD + [dict(eps=[0.0, 7.0]), dict(eps=[7.0], eps_g=FAKE)]:
        add("thrl_sampled_chain", SC.sc_args, dict(g, **kw), cfg="forty" if kw.get("n_tuples") == 21 * 40 else "base")
    tuple_counts("thrl_sampled_chain", SC.sc_args, g, dict(n_prices=1))
    tuple_kinds("thrl_sampled_chain", SC.sc_args, g, dict(n_tuples=21 * 40, n_prices=21))
    add("thrl_sampled_chain", SC.sc_args, dict(g, n_tuples=1024, n_prices=1024), cfg="sp_big")
    for f in SC.SC_REQUIRED:
        add("thrl_sampled_chain", SC.sc_args, dict(g, **{f: None}))
    add("thrl_sampled_chain", SC.sc_args, dict(g, prob=[None, None]))
    add("thrl_sampled_chain", SC.sc_args, dict(flags=1))
    nulls("thrl_sampled_chain", SC.sc_args, g)
    for kw in SN.SN_BAD + [dict(n_nodes=4097), dict(noise_prob=7.0, noise_prob_g=FAKE), dict(eps=[7.0], eps_g=FAKE)]:
        add("thrl_sampled_noise_chain", SN.sn_args, dict(g, **kw))
    tuple_counts("thrl_sampled_noise_chain", SN.sn_args, g, dict(n_prices=1))
    tuple_kinds("thrl_sampled_noise_chain", SN.sn_args, g, dict(n_tuples=21 * 40, n_prices=21))
    add("thrl_sampled_noise_chain", SN.sn_args, dict(g, n_tuples=1024, n_prices=1024, n_nodes=4096), cfg="sp_big")
    for f in SN.SN_REQUIRED:
        add("thrl_sampled_noise_chain", SN.sn_args, dict(g, **{f: None}))
    add("thrl_sampled_noise_chain", SN.sn_args, dict(g, nprob=[None, None]))
    add("thrl_sampled_noise_chain", SN.sn_args, dict(flags=1))
    nulls("thrl_sampled_noise_chain", SN.sn_args, g)

    # ---- thrl_sampled_response, thrl_sampled_response_noise, thrl_sampled_deviation, thrl_sampled_deviation_noise: the
    # tables of their own host tests, the cases those tests accept up to a missing pointer, and the working set's edge
    def sampled(entry, build, g, bad, fine, required, rows, big, ws):
        for kw in bad + fine:
            add(entry, build, dict(g, **kw), cfg="forty" if kw.get("n_tuples") == 21 * 40 else "base")
        tuple_counts(entry, build, g, dict(n_prices=1))
        tuple_kinds(entry, build, g, dict(n_tuples=21 * 40, n_prices=21))
        shape = dict(n_tuples=ws["T"], n_prices=ws["D"], **({"n_nodes": ws["Jn"]} if "Jn" in ws else {}))
        add(entry, build, dict(g, **shape), cfg=big)
        for f in required:
            add(entry, build, dict(g, **{f: None}))
        for r in rows:
            add(entry, build, dict(g, **{r: [None, None]}))
        nulls(entry, build, g)

    g = dict(loss_all=None)
    fine = [dict(agents=1, gamma=[0.5, 7.0]), dict(eps=[0.0, 7.0]), dict(gamma=[7.0], sweep_gamma=FAKE), dict(eps=[7.0], eps_g=FAKE)]
    sampled("thrl_sampled_response", SR.sr_args, g, SR.SR_BAD, fine, SR.SR_REQUIRED, ("prob",), "sr_big",
            SR.sr.working_set(SDN._shape(26, 32)))
    sampled("thrl_sampled_response_noise", SRN.srn_args, g, SRN.SRN_BAD,
            fine + [dict(noise_prob=7.0, noise_prob_g=FAKE), dict(n_nodes=4097)], SRN.SRN_INPUTS + SRN.SRN_OUTPUTS, ("prob", "nprob"),
            "srn_big", SRN.sr.working_set_noise(SDN._shape(35, 21)))
    for entry, build, weighted in (("thrl_sampled_response", SR.sr_args, SR.SR_WEIGHTED),
                                   ("thrl_sampled_response_noise", SRN.srn_args, SRN.SRN_WEIGHTED)):
        for f in weighted:
            add(entry, build, dict({w: FAKE for w in weighted}, pi=FAKE, **{f: None}))
    g = dict(mass=None)
    fine = [dict(flags=1, dev_action=3), dict(gamma=0.0), dict(gamma=1.0), dict(eps=[0.0, 7.0]), dict(gamma=7.0, sweep_gamma=FAKE),
            dict(eps=[7.0], eps_g=FAKE), dict(dev_action=20, deviator=0), dict(row_begin=29, row_count=3), dict(flags=1, dev_policy=FAKE),
            dict(dev_len=32), dict(flags=1)]
    sampled("thrl_sampled_deviation", SD.sd_args, g, SD.SD_BAD, fine, SD.SD_TABLES + SD.SD_OUTPUTS, ("prob",), "sd_big",
            SD.sd.working_set(SDN._shape(35, 32)))
    sampled("thrl_sampled_deviation_noise", SDN.sdn_args, g, SDN.SDN_BAD,
            fine + [dict(noise_prob=0.0), dict(noise_prob=1.0), dict(noise_prob=7.0, noise_prob_g=FAKE), dict(n_nodes=2, band_w=1),
                    dict(n_nodes=4097)], SDN.SDN_TABLES + SDN.SDN_OUTPUTS, ("prob", "nprob"), "sdn_big",
            SDN.sd.working_set_noise(SDN._shape(35, 28)))

    # ---- thrl_equilibrium, thrl_attractors, thrl_stationary: their plan and their limits come before the other checks
    g = dict(v_on=None)
    for kw in _bad(EQ.test_bad_arguments_are_bad_config):
        add("thrl_equilibrium", EQ._args, dict(g, **kw))
    for kw, cfg in ((dict(), "gamma_one"), (dict(), "gamma_nan"), (dict(agents=1), "gamma_one"), (dict(sweep_gamma=FAKE), "gamma_one"),
                    (dict(), "eq_wide"), (dict(), "eq_fine")):
        add("thrl_equilibrium", EQ._args, dict(g, **kw), cfg=cfg)
    for f in _bad(EQ.test_missing_outputs_are_null):
        if f not in ("q", "args"):
            add("thrl_equilibrium", EQ._args, dict(g, **{f: None}))
    add("thrl_equilibrium", EQ._args, {}, q=None, ident="q=None")
    nulls("thrl_equilibrium", EQ._args, g)
    for kw in _bad(AT.test_bad_arguments_are_bad_config):
        add("thrl_attractors", AT._starts_args, dict(kw, reset_reward=None), q=None)
    for cfg in ("eq_wide", "eq_fine"):
        add("thrl_attractors", AT._args, {}, cfg=cfg, q=None)
    for f in ("state0", "policy") + AT.OUTPUTS + AT.RESET:
        add("thrl_attractors", AT._starts_args, {f: None}, q=None)
    add("thrl_attractors", AT._args, {}, q=None, ident="q=None")
    add("thrl_attractors", AT._args, dict(n_starts=101), q=None)
    add("thrl_attractors", AT._args, dict(flags=1, n_attr=None), q=None)
    nulls("thrl_attractors", AT._args, q=None)
    for kw in _bad(ST.test_bad_arguments_are_bad_config) + [dict(n_cells=4097), dict(n_cells=3500), dict(n_cells=3001),
                                                           dict(noise_prob=0.0, noise_prob_g=FAKE)]:
        add("thrl_stationary", ST._args, kw, q=None)
    add("thrl_stationary", ST._args, {}, cfg="eq_wide", q=None)
    for f in ("policy",) + ST.TABLES + ST.OUTPUTS:
        add("thrl_stationary", ST._args, {f: None}, q=None)
    add("thrl_stationary", ST._args, dict(flags=2), q=None)
    add("thrl_stationary", ST._args, dict(flags=1, mass=None), q=None)
    add("thrl_stationary", ST._args, {}, q=None, ident="q=None")
    nulls("thrl_stationary", ST._args, q=None)

    # ---- thrl_qtable_episodes, thrl_mixed_episodes: injection past what an int8 choice holds
    for cfg in ("inj_wide", "inj_wide_second"):
        add("thrl_qtable_episodes", _episode_buffers, {}, cfg=cfg)
        add("thrl_mixed_episodes", _mixed_args, {}, cfg=cfg)
    add("thrl_mixed_episodes", _mixed_args, dict(kind=(0, 1)), cfg="inj_wide")
    add("thrl_mixed_episodes", _mixed_args, dict(kind=(1, 0)), cfg="inj_wide_second")
    return out


def run(lib):
    """[[entry point, case id, return code, message]] in the order of cases()."""
    from th_rl_amd import _lib
    cfgs = {k: _lib.cfg_from_config(v, 64, 0)[0] for k, v in CONFIGS.items()}
    rows = []
    for entry, ident, cfg, q, a in cases():
        if a is not None:             # no case may have every pointer of the last NULL check set
            assert not all(_set(v) for v in LAST_NULL[entry](a, q)), (entry, ident)
        pa = None if a is None else ctypes.byref(a)
        if entry == "thrl_group_stats":
            rc = lib.thrl_group_stats(pa, None)
        elif entry in ("thrl_qtable_episodes", "thrl_mixed_episodes"):
            r = _lib.Run()
            r.n_episodes = 1
            fake = ctypes.c_void_p(FAKE)
            rc = (lib.thrl_qtable_episodes(ctypes.byref(cfgs[cfg]), pa, ctypes.byref(r), None) if entry == "thrl_qtable_episodes"
                  else lib.thrl_mixed_episodes(ctypes.byref(cfgs[cfg]), pa, fake, fake, fake, ctypes.byref(r), fake, fake, None))
        else:
            pc = None if cfg is None else ctypes.byref(cfgs[cfg])
            fn = getattr(lib, entry)
            rc = fn(pc, ctypes.c_void_p(q), pa, None) if entry in TAKES_Q else fn(pc, pa, None)
        rows.append([entry, ident, rc, lib.thrl_last_error().decode("ascii", "replace")])
    return rows


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def rows(lib):
    return run(lib)


def test_every_refusal_keeps_its_code_and_its_words(rows):
    golden = json.load(open(GOLDEN))
    assert [r[:2] for r in rows] == [r[:2] for r in golden]
    diff = [(got, want) for got, want in zip(rows, golden) if got != want]
    assert not diff, diff[:5]


def test_the_recorded_table_holds_refusals_only():
    golden = json.load(open(GOLDEN))
    assert {r[2] for r in golden} == {-1, -2, -3}
    assert {r[0] for r in golden} == set(LAST_NULL)
    assert all(r[3] for r in golden)


# fail( sites of thrl_api_analysis.hip that no case reaches, by the start of their format string
UNREACHED = {
    # their own comment says they cannot happen within the limits (and they follow the device query)
    "thrl_tuple_equilibrium: %d bytes of LDS per game, the device has", "thrl_tuple_attractors: %d bytes of LDS per game, the device has",
    "thrl_tuple_stationary: %d bytes of LDS per game", "thrl_equilibrium: %d bytes of LDS per game",
    # behind the entry point's first HIP call
    "thrl_sampled_chain: %d bytes of LDS per game (T=%d, n_prices=%d), the device has",
    "thrl_sampled_noise_chain: %d bytes of LDS per game (T=%d, n_prices=%d, n_nodes=%d), the device has",
    "thrl_attractors: %lld bytes of LDS per game",
    # thrl_group_stats past its NULL check: they read group_of on the host and need every pointer set, which no case
    # of this module may have
    "group_of[%d]=%d out of", "quantity %d: range", "quantity %d: inv_w", "quantity %d: scale[%d]=%g must be a power of two with ",
}


def test_every_fail_site_before_the_first_hip_call_is_reached():
    """Every format string of a fail( in thrl_api_analysis.hip matches a recorded message, but for UNREACHED."""
    src = open(os.path.join(CSRC, "thrl_api_analysis.hip")).read()
    sites = re.findall(r'\bfail\(THRL_ERR_\w+,\s*"((?:[^"\\]|\\.)*)"', src)
    assert len(sites) > 60
    messages = {r[3] for r in json.load(open(GOLDEN))}
    missed = []
    for fmt in sites:
        if any(fmt.startswith(u) for u in UNREACHED):
            continue
        pat = re.compile("^" + ".*".join(re.escape(p) for p in re.split(r"%(?:lld|[dgsx])", fmt)))
        if not any(pat.match(m) for m in messages):
            missed.append(fmt)
    assert not missed, missed


# a fragment of each message of a check that several entry points share -> the entry points that make that check
_TUPLE_COUNT = ("thrl_tuple_policy thrl_tuple_walk thrl_tuple_deviation thrl_tuple_equilibrium thrl_tuple_attractors "
                "thrl_tuple_stationary thrl_sampled_chain thrl_sampled_noise_chain")
_TUPLE_KINDS = "thrl_tuple_policy thrl_price_policy thrl_tuple_stationary thrl_price_probs thrl_sampled_chain thrl_sampled_noise_chain"
_WALKS = "thrl_deviation thrl_crossplay thrl_tuple_walk thrl_tuple_deviation"
_CHAINS = "thrl_tuple_stationary thrl_sampled_chain thrl_sampled_noise_chain thrl_stationary"
SHARED = {
    "n_games=65 out of [1,64]": "thrl_deviation thrl_policy_track thrl_crossplay thrl_tuple_policy thrl_price_policy thrl_price_probs "
                                "thrl_equilibrium thrl_attractors thrl_stationary",
    "n_games=0 must be >= 1": "thrl_group_stats thrl_tuple_walk thrl_tuple_deviation thrl_tuple_equilibrium thrl_tuple_attractors "
                              "thrl_tuple_stationary thrl_sampled_chain thrl_sampled_noise_chain",
    "horizon=0 out of": _WALKS, "rows [": _WALKS, "n_steps=-1 out of [0,": "thrl_crossplay thrl_tuple_walk",
    "deviator=": "thrl_deviation thrl_tuple_deviation", "dev_len=0": "thrl_deviation thrl_tuple_deviation",
    "out of [dev_len=": "thrl_deviation thrl_tuple_deviation", "dev_action=": "thrl_deviation thrl_tuple_deviation",
    "max_iters=0 out of": _CHAINS, "tol=nan": _CHAINS, "eps[0]=": "thrl_sampled_chain thrl_sampled_noise_chain",
    "agents=0x0": "thrl_tuple_equilibrium thrl_equilibrium", "gamma=1:": "thrl_tuple_equilibrium thrl_equilibrium",
    "n_tuples=0 must be": _TUPLE_COUNT, "n_tuples=4097, at most": _TUPLE_COUNT, "is not the product": _TUPLE_COUNT,
    "is a CAC agent": _TUPLE_KINDS, ": kind=4": _TUPLE_KINDS, "neural agent 1: actions=40": _TUPLE_KINDS,
    "nn_params[1] is NULL": "thrl_tuple_policy thrl_price_policy", "q is NULL with a QTable agent": "thrl_tuple_policy thrl_price_policy",
}


def test_a_shared_check_is_reached_through_every_entry_point_that_makes_it():
    golden = json.load(open(GOLDEN))
    missed = [(frag, entry) for frag, entries in SHARED.items() for entry in entries.split()
              if not any(r[0] == entry and frag in r[3] for r in golden)]
    assert not missed, missed


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_api_refusals_host.py --record")
    from th_rl_amd import _lib
    table = run(_lib.load())
    with open(GOLDEN, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in table) + "\n]\n")
    print("recorded %d cases from %s" % (len(table), _lib.LIB_PATH))
