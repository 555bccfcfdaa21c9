"""Helpers of the parity-mode tests of mixed games (fixtures G12, tests/golden/make_golden_mixed_run.py): the fixture
as injection arrays, and the composed oracle -- the loop of test_gpu_nn.py's
test_qtable_vs_reinforce_game_against_composed_oracle (oracle.oracle for env / encode / TD, oracle.nn_oracle for the
network update) written to take injected draws and actions instead of Philox draws and a sampled policy.  No GPU."""
import json
import os

import numpy as np

from oracle import nn_oracle as NN
from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {"reinforce": "g12_mixed_run_reinforce.npz", "actorcritic": "g12_mixed_run_actorcritic.npz",
            "noise_swapped": "g12_mixed_run_noise_swapped.npz"}
NN_DEFAULTS = dict(gamma=0.98, capacity=50000, min_memory=1000, entropy=0)     # agents.py:119-131, 222-233


class Fixture:
    def __init__(self, name):
        d = np.load(os.path.join(GOLDEN, FIXTURES[name]))
        self.d = d
        self.config = json.loads(str(d["config_json"]))
        self.qi, self.ni, self.kind = int(d["qtable_index"]), int(d["nn_index"]), str(d["nn_kind"])
        self.E, self.T = d["u"].shape
        self.A = int(self.config["agents"][self.ni]["actions"])
        self.noise = float(self.config["environment"]["noise_prob"]) > 0
        self.nn = dict(NN_DEFAULTS, **self.config["agents"][self.ni])
        self.updates = [int(e) for e in d["nn_update_episode"]]

    def inj(self, G=1, game=0, e0=0, e1=None, seed=1234):
        """Injection arrays [E, T, 2, G] / [E, T, G] for episodes [e0, e1): the fixture's streams in column `game`, other
        draws (valid, but different) in the other games; slots that are not read hold values that would break a run
        that read them."""
        e1 = self.E if e1 is None else e1
        d, E, T = self.d, e1 - e0, self.T
        rs = np.random.RandomState(seed)
        Aq = int(self.config["agents"][self.qi]["actions"])
        u = np.full((self.E, T, 2, G), np.nan)
        ch = np.full((self.E, T, 2, G), -7, np.int8)
        ac = np.full((self.E, T, 2, G), -9, np.int8)
        u[:, :, self.qi, :] = rs.uniform(0, 1, (self.E, T, G))
        ch[:, :, self.qi, :] = rs.randint(0, Aq, (self.E, T, G))
        ac[:, :, self.ni, :] = rs.randint(0, self.A, (self.E, T, G))
        nu = rs.uniform(0, 1, (self.E, T, G))
        na = rs.uniform(7.0, 10.0, (self.E, T, G))
        u[:, :, self.qi, game], ch[:, :, self.qi, game], ac[:, :, self.ni, game] = d["u"], d["choice"], d["nn_action"]
        nu[:, :, game], na[:, :, game] = d["noise_u"], d["noise_a"]
        out = dict(u=u[e0:e1], choice=ch[e0:e1], action=ac[e0:e1])
        if self.noise:
            out.update(noise_u=nu[e0:e1], noise_a=na[e0:e1])
        assert out["u"].shape == (E, T, 2, G)
        return out


def composed_oracle(config, table, state0, w0, inj, game=0):
    """trainer.train_one's loop (trainer.py:45-70) for one game of a two-agent QTable / Reinforce|ActorCritic pairing,
    played from injected draws and actions.  Returns prices, rewards, scaled actions per step, the two log arrays,
    epsilon per episode, the final table and counter, and the network parameters after each update."""
    kinds = [a.get("name", "QTable") for a in config["agents"]]
    qi = kinds.index("QTable"); ni = 1 - qi
    qa = dict(O.QTABLE_DEFAULTS, **config["agents"][qi])
    na = dict(NN_DEFAULTS, **config["agents"][ni])
    A, Aq = int(na["actions"]), int(qa["actions"])
    slot = dict(name="QTable", states=1, actions=A, action_range=na["action_range"])
    agents = [None, None]
    agents[qi], agents[ni] = config["agents"][qi], slot
    qcfg, _ = O.cfg_from_config({"agents": agents, "environment": config["environment"]}, 1, 1)
    T = int(config["environment"]["max_steps"])
    noise_prob = float(qcfg.noise_prob)
    E = inj["action"].shape[0]
    table = np.array(table, np.float64).copy(); counter = np.zeros(table.shape, np.int32)
    w = np.array(w0, np.float32).copy(); m = np.zeros_like(w); v = np.zeros_like(w); step = 0
    price, eps = float(state0), float(qa["epsilon"])
    memq, memn = [], []
    prices = np.zeros((E, T)); rewards = np.zeros((E, T, 2)); scaled = np.zeros((E, T, 2))
    rlog = np.zeros((E, 2)); alog = np.zeros((E, 2)); eps_log = np.zeros(E); ws = []; upd = []
    lo_q, hi_q = qa["action_range"]; lo_n, hi_n = na["action_range"]
    for e in range(E):
        for t in range(T):
            if inj["u"][e, t, qi, game] < eps:
                aq = int(inj["choice"][e, t, qi, game])
            else:
                aq = int(np.argmax(table[O.encode32(price, qa["max_state"], qa["states"])]))
            an = int(inj["action"][e, t, ni, game])
            sc = [0.0, 0.0]
            sc[qi], sc[ni] = O.scale(aq, Aq, lo_q, hi_q), NN.scale(an, A, lo_n, hi_n)
            noisy = noise_prob > 0 and inj["noise_u"][e, t, game] < noise_prob
            nprice, rew = O.env_step(qcfg, sc, noisy=bool(noisy), new_a=float(inj["noise_a"][e, t, game]) if noisy else 0.0)
            memq.append((O.encode64(price, qa["max_state"], qa["states"]), aq, rew[qi],
                         O.encode64(nprice, qa["max_state"], qa["states"])))
            memn.append((price, an, rew[ni], nprice))
            rlog[e] += rew / T; alog[e] += np.array(sc) / T
            prices[e, t], rewards[e, t], scaled[e, t] = nprice, rew, sc
            price = nprice
        memq = memq[-int(qa["capacity"]):]
        trained = []
        for i in range(2):                                   # [A.train_net() for A in agents], in seat order
            if i == qi:
                if len(memq) >= int(qa["min_memory"]):
                    st, ac, rw, ns = zip(*memq)
                    O.td_update(table, counter, st, ac, rw, ns, float(qa["alpha"]), float(qa["gamma"])); memq = []
                eps = float(qa["eps_end"]) + (eps - float(qa["eps_end"])) * float(qa["eps_step"])
            elif len(memn) >= int(na["min_memory"]):
                pr, ac, rw, npz = zip(*memn)
                if kinds[ni] == "ActorCritic":
                    # the [N, N] advantage built as torch builds it (explicit=True): the closed-form row / column sums of
                    # ac_train_net round differently, which moves one near-zero-gradient element by 4.9e-6 in Adam's
                    # first step on G12; the explicit form stays within 6e-8 of the reference
                    g, _ = NN.ac_gradients(w, A, pr, ac, rw, npz, float(na["gamma"]), float(na["entropy"]), explicit=True)
                    w, m, v, step = NN.adam_step(np.asarray(w, np.float32), g, np.asarray(m, np.float32),
                                                 np.asarray(v, np.float32), step)
                else:
                    w, m, v, step, _ = NN.train_net(w, m, v, step, A, pr, ac, rw, float(na["gamma"]), float(na["entropy"]))
                memn = []; ws.append(np.array(w).copy()); upd.append(e)
        eps_log[e] = eps
    return dict(prices=prices, rewards=rewards, scaled=scaled, rewards_log=rlog, actions_log=alog, eps=eps_log,
                table=table, counter=counter, nn_w=np.stack(ws) if ws else np.zeros((0, len(w))), updates=upd)
