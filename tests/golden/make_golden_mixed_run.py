#!/usr/bin/env python3
"""Fixture G12: full training runs of the REFERENCE with a neural agent in the game (QTable vs Reinforce, the
shipped example_config.json; the same with ActorCritic; Reinforce vs QTable with env noise), with every random
quantity the trajectory depends on recorded, so the run can be replayed draw for draw (parity mode of
thrl_mixed_episodes / MixedGameBatch.run(inj=...)).  Data only.
Usage: python tests/golden/make_golden_mixed_run.py [--out DIR]

The reference never seeds anything; this harness seeds numpy.random / random / torch and pins torch to one
thread, then calls the reference's own train_one (trainer.py:45-70 is the loop).  Recorded per file:
  * config_json, seed, qtable_index / nn_index (the two seats), nn_kind;
  * init_table [(S+1), A] and state0 (reset(), trainer.py:45); nn_w0 = the initial network parameters in the
    thrl_nn_init layout [fc1.weight | fc1.bias | fc_pi.weight row-major | fc_pi.bias ( | fc_v.weight | fc_v.bias)];
  * u, choice [E, T]: the QTable agent's random.uniform / random.choice per step (agents.py:81-82), choice = -1
    where it did not explore;
  * nn_action [E, T]: what the neural agent's sample_action returned (Categorical.sample().item(), agents.py:160-163
    / 270-273);
  * noise_u, noise_a [E, T]: the env's two numpy.random.uniform draws (environments.py:28-29), noise_a = NaN where
    the intercept was not redrawn;
  * states [E, T] (price after the step), rewards, scaled_actions [E, T, 2];
  * rewards_log, actions_log [E, 2] (trainer.py:65-66, from log.csv), eps [E] after each QTable.train_net;
  * final_table, final_counter; nn_update_episode [K] and nn_w [K, P]: the parameters after each network update.

Third case: the QTable agent gets min_memory = max_steps so that it trains at every episode end, which is what the
tuple-chain episode kernel takes; the Reinforce agent's min_memory = 50 gives an update every second episode.
"""
import json
import os
import random
import sys
import tempfile

import numpy

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
CONFIG = os.path.join(REF, "th_rl", "some_path", "configs", "example_config.json")

sys.dont_write_bytecode = True
sys.path.insert(0, REF)

import torch  # noqa: E402
import pandas  # noqa: E402
import th_rl.trainer as ref_trainer  # noqa: E402
import th_rl.agents as ref_agents  # noqa: E402
import th_rl.environments as ref_env  # noqa: E402

NN_PARAMS = {"Reinforce": ["fc1.weight", "fc1.bias", "fc_pi.weight", "fc_pi.bias"],
             "ActorCritic": ["fc1.weight", "fc1.bias", "fc_pi.weight", "fc_pi.bias", "fc_v.weight", "fc_v.bias"]}


def flat(agent, kind):
    sd = agent.state_dict()
    return numpy.concatenate([sd[k].detach().numpy().ravel() for k in NN_PARAMS[kind]]).astype("float32")


def run_reference(config, seed):
    kinds = [a["name"] for a in config["agents"]]
    qi = kinds.index("QTable")
    ni = 1 - qi
    kind = kinds[ni]
    E, T = config["training"]["epochs"], config["environment"]["max_steps"]
    nn_cls = getattr(ref_agents, kind)
    rec = dict(u=[], choice=[], nn_action=[], noise_u=[], noise_a=[], acts=[], states=[], rewards=[], eps=[],
               nn_w=[], nn_update_episode=[], in_step=False, episode=0)
    captured = {}
    orig = dict(uniform=random.uniform, choice=random.choice, np_uniform=numpy.random.uniform,
                step=ref_env.NoisyPriceState.step, q_train=ref_agents.QTable.train_net,
                nn_sample=nn_cls.sample_action, nn_train=nn_cls.train_net, create=ref_trainer.create_game)

    def uniform(a, b):
        v = orig["uniform"](a, b)
        rec["u"].append(v); rec["choice"].append(-1)
        return v

    def choice(seq):
        v = orig["choice"](seq)
        rec["choice"][-1] = int(v)
        return v

    def np_uniform(lo=0.0, hi=1.0, size=None):
        v = orig["np_uniform"](lo, hi, size)
        if rec["in_step"]:
            if lo == 0 and hi == 1:
                rec["noise_u"].append(float(v)); rec["noise_a"].append(float("nan"))
            else:
                rec["noise_a"][-1] = float(v)
        return v

    def step(env, actions):
        rec["in_step"] = True
        try:
            out = orig["step"](env, actions)
        finally:
            rec["in_step"] = False
        rec["acts"].append([float(a) for a in actions])
        rec["states"].append(float(out[0][0]))
        rec["rewards"].append([float(r) for r in out[1]])
        return out

    def q_train(agent):
        orig["q_train"](agent)
        rec["eps"].append(float(agent.epsilon))

    def nn_sample(agent, state):
        v = orig["nn_sample"](agent, state)
        rec["nn_action"].append(int(v))
        return v

    def nn_train(agent):
        due = len(agent.memory) >= agent.min_memory
        orig["nn_train"](agent)
        if due:
            rec["nn_w"].append(flat(agent, kind)); rec["nn_update_episode"].append(rec["episode"])
        rec["episode"] += 1

    def create_game(path):
        cfg, agents, env = orig["create"](path)
        captured["table"] = agents[qi].table.copy()
        captured["w0"] = flat(agents[ni], kind)
        orig_reset = env.reset

        def reset():
            s = orig_reset()
            captured["state0"] = float(s[0])
            return s
        env.reset = reset
        return cfg, agents, env

    with tempfile.TemporaryDirectory() as tmp:
        cpath = os.path.join(tmp, "cfg.json")
        with open(cpath, "w") as f:
            json.dump(config, f)
        exp = os.path.join(tmp, "run")
        numpy.random.seed(seed); random.seed(seed); torch.manual_seed(seed)
        random.uniform, random.choice, numpy.random.uniform = uniform, choice, np_uniform
        ref_env.NoisyPriceState.step = step
        ref_agents.QTable.train_net = q_train
        nn_cls.sample_action, nn_cls.train_net = nn_sample, nn_train
        ref_trainer.create_game = create_game
        try:
            ref_trainer.train_one(exp, cpath)
        finally:
            random.uniform, random.choice, numpy.random.uniform = orig["uniform"], orig["choice"], orig["np_uniform"]
            ref_env.NoisyPriceState.step = orig["step"]
            ref_agents.QTable.train_net = orig["q_train"]
            nn_cls.sample_action, nn_cls.train_net = orig["nn_sample"], orig["nn_train"]
            ref_trainer.create_game = orig["create"]
        final_table = numpy.load(os.path.join(exp, "%d.npy" % qi))
        final_counter = numpy.load(os.path.join(exp, "%d_counter.npy" % qi))
        log = pandas.read_csv(os.path.join(exp, "log.csv"), header=[0, 1], float_precision="round_trip")
        rewards_log = log["rewards"].to_numpy(dtype="float64")
        actions_log = log["actions"].to_numpy(dtype="float64")

    return dict(
        seed=numpy.int64(seed), config_json=numpy.array(json.dumps(config)),
        qtable_index=numpy.int64(qi), nn_index=numpy.int64(ni), nn_kind=numpy.array(kind),
        init_table=captured["table"], state0=numpy.float64(captured["state0"]), nn_w0=captured["w0"],
        u=numpy.array(rec["u"], "float64").reshape(E, T), choice=numpy.array(rec["choice"], "int8").reshape(E, T),
        nn_action=numpy.array(rec["nn_action"], "int8").reshape(E, T),
        noise_u=numpy.array(rec["noise_u"], "float64").reshape(E, T),
        noise_a=numpy.array(rec["noise_a"], "float64").reshape(E, T),
        states=numpy.array(rec["states"], "float64").reshape(E, T),
        rewards=numpy.array(rec["rewards"], "float64").reshape(E, T, 2),
        scaled_actions=numpy.array(rec["acts"], "float64").reshape(E, T, 2),
        rewards_log=rewards_log, actions_log=actions_log, eps=numpy.array(rec["eps"], "float64").reshape(E),
        final_table=final_table, final_counter=final_counter,
        nn_update_episode=numpy.array(rec["nn_update_episode"], "int64"),
        nn_w=numpy.stack(rec["nn_w"]).astype("float32"))


def cases():
    base = json.load(open(CONFIG))
    base["training"] = {"print_freq": 10 ** 9, "epochs": 30}
    yield "g12_mixed_run_reinforce.npz", base, 5
    ac = json.loads(json.dumps(base))
    ac["agents"][1]["name"] = "ActorCritic"
    ac["training"]["epochs"] = 20
    yield "g12_mixed_run_actorcritic.npz", ac, 5
    T = 25
    sw = json.loads(json.dumps(base))
    sw["agents"] = [dict(base["agents"][1], min_memory=50), dict(base["agents"][0], min_memory=T)]
    sw["environment"].update(noise_prob=0.5, max_steps=T)
    sw["training"]["epochs"] = 8
    yield "g12_mixed_run_noise_swapped.npz", sw, 7


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE
    torch.set_num_threads(1)
    for name, config, seed in cases():
        d = run_reference(config, seed)
        p = os.path.join(out, name)
        numpy.savez_compressed(p, **d)
        print("wrote", p, os.path.getsize(p), "bytes; network updates at episodes", d["nn_update_episode"].tolist())


if __name__ == "__main__":
    main()
