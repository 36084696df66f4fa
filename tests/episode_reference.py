"""Plain numpy / Python restatement of the episode accounts of stable_baselines3 2.3.2 that
csrc/episode.hip keeps on the device (restated from SB3's published code; SB3 is not installed):

* ``evaluation.py::evaluate_policy``'s accounting: ``episode_count_targets``, float64
  ``current_rewards`` / int ``current_lengths``, the ``for i in range(n_envs)`` loop that appends to
  ``episode_rewards`` / ``episode_lengths`` while ``episode_counts[i] < episode_count_targets[i]``;
* the Monitor window ``ep_info_buffer = deque(maxlen=stats_window_size)`` of
  ``on_policy_algorithm.py`` (every finished episode of every env, in env order within a step);
* ``utils.safe_mean`` and ``np.std``.

The yardstick of tests/test_episode_gpu.py and tests/test_evaluate_policy_gpu.py; pinned on a case
computed by hand in tests/test_episode_abi.py.
"""
from collections import deque

import numpy as np


def episode_count_targets(n_eval_episodes, n_envs):
    return np.array([(n_eval_episodes + i) // n_envs for i in range(n_envs)], dtype="int")


def safe_mean(arr):
    return np.nan if len(arr) == 0 else float(np.mean(arr))


class Accounts:
    """One object for the three log forms: ``quota`` (evaluate_policy's targets) or None (Monitor:
    every episode), ``ring`` True: deque(maxlen=capacity), False: a list of the first ``capacity``
    episodes, later ones counted in ``dropped``."""

    def __init__(self, n_envs, capacity, ring, quota=None):
        self.n_envs, self.capacity, self.ring = n_envs, capacity, ring
        self.quota = None if quota is None else np.asarray(quota, dtype="int")
        self.current_rewards = np.zeros(n_envs)              # float64, as SB3's
        self.current_lengths = np.zeros(n_envs, dtype="int")
        self.episode_counts = np.zeros(n_envs, dtype="int")
        self.log = deque(maxlen=capacity) if ring else []    # (return, length, env)
        self.total = self.steps = self.dropped = 0

    def step(self, rewards, term, trunc):
        self.current_rewards += np.asarray(rewards, np.float32).astype(np.float64)
        self.current_lengths += 1
        for i in range(self.n_envs):
            if self.quota is not None and not self.episode_counts[i] < self.quota[i]:
                continue
            if term[i] or trunc[i]:
                entry = (float(self.current_rewards[i]), int(self.current_lengths[i]), i)
                if self.ring or len(self.log) < self.capacity:
                    self.log.append(entry)
                else:
                    self.dropped += 1
                self.total += 1
                self.episode_counts[i] += 1
                self.current_rewards[i] = 0
                self.current_lengths[i] = 0
        self.steps += 1

    @property
    def remaining(self):
        return 0 if self.quota is None else int(np.maximum(self.quota - self.episode_counts, 0).sum())

    def episodes(self):
        r = np.array([e[0] for e in self.log], np.float64)
        n = np.array([e[1] for e in self.log], np.int32)
        i = np.array([e[2] for e in self.log], np.int32)
        return r, n, i

    def summary(self):
        r, n, _ = self.episodes()
        nan = np.nan
        return {"n": float(len(r)), "ep_rew_mean": safe_mean(r), "ep_rew_std": float(np.std(r)) if len(r) else nan,
                "ep_rew_min": float(r.min()) if len(r) else nan, "ep_rew_max": float(r.max()) if len(r) else nan,
                "ep_len_mean": safe_mean(n), "ep_len_std": float(np.std(n.astype(np.float64))) if len(r) else nan,
                "total": float(self.total)}


def evaluate_policy_accounts(step_fn, n_envs, n_eval_episodes):
    """evaluate_policy's loop around ``step_fn(t) -> (rewards, term, trunc)`` (host arrays of one
    env.step): runs until every target is met -> (episode_rewards, episode_lengths, steps taken)"""
    acc = Accounts(n_envs, n_eval_episodes, False, episode_count_targets(n_eval_episodes, n_envs))
    t = 0
    while (acc.episode_counts < acc.quota).any():
        acc.step(*step_fn(t))
        t += 1
    r, n, _ = acc.episodes()
    return [float(x) for x in r], [int(x) for x in n], t


def stream(T, E):
    """the constructed inputs of tests/test_episode_gpu.py: done[t][e] = ((t + 1) % (2 + e % 7) == 0),
    term on even envs, trunc on odd ones, rew = float32(((31 t + 17 e) % 64 - 20) / 8): exact in float32,
    every partial sum exact in float64"""
    t = np.arange(T)[:, None]
    e = np.arange(E)[None, :]
    done = (t + 1) % (2 + e % 7) == 0
    term = done & (e % 2 == 0)
    trunc = done & (e % 2 == 1)
    rew = (((31 * t + 17 * e) % 64 - 20) / 8).astype(np.float32)
    return rew, term, trunc
