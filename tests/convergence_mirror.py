"""numpy restatement of thrl_policy_track (include/thrl.h), written from the definitions: the greedy policy of every
row of every agent (numpy.argmax: the first maximum), compared at checks, stable_since / changes / converged_at /
conv_since per game, and the snapshot of the tables and state at convergence."""
import numpy as np


def policy_of(q, shapes, offsets):
    """[G, P] uint16: argmax of every row (agent 0's rows first) of q [G, stride]."""
    q = np.asarray(q)
    cols = []
    for (r, a), o in zip(shapes, offsets):
        cols.append(np.argmax(q[:, o:o + r * a].reshape(q.shape[0], r, a), axis=2))
    return np.concatenate(cols, axis=1).astype(np.uint16)


class Mirror:
    def __init__(self, q, shapes, offsets, episode, window, state=None, snapshot=False):
        self.shapes, self.offsets, self.window, self.snapshot = shapes, offsets, int(window), snapshot
        self.policy = policy_of(q, shapes, offsets)
        G = self.policy.shape[0]
        self.stable_since = np.full(G, int(episode), np.int64)
        self.converged_at = np.full(G, -1, np.int64)
        self.conv_since = np.full(G, -1, np.int64)
        self.changes = np.zeros(G, np.int32)
        self.n_converged = 0
        if snapshot:
            self.q_conv = np.zeros_like(np.asarray(q))
            self.state_conv = np.zeros(G, np.float64)

    def check(self, q, episode, state=None):
        e = int(episode)
        pol = policy_of(q, self.shapes, self.offsets)
        changed = np.any(pol != self.policy, axis=1)
        self.policy[changed] = pol[changed]
        self.stable_since[changed] = e
        self.changes[changed] += 1
        new = (self.converged_at < 0) & (e - self.stable_since >= self.window)
        self.converged_at[new] = e
        self.conv_since[new] = self.stable_since[new]
        self.n_converged += int(new.sum())
        if self.snapshot:
            self.q_conv[new] = np.asarray(q)[new]
            self.state_conv[new] = np.asarray(state)[new]
        return self.n_converged

    def arrays(self):
        out = dict(policy=self.policy.copy(), stable_since=self.stable_since.copy(), converged_at=self.converged_at.copy(),
                   conv_since=self.conv_since.copy(), changes=self.changes.copy())
        if self.snapshot:
            out.update(q_conv=self.q_conv.copy(), state_conv=self.state_conv.copy())
        return out
