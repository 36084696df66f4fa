"""On-device episode statistics, ``evaluate_policy`` and the evaluation callback (the rest of
examples/learn.py:72-94, 142 next to ``RolloutCollector`` and ``PPOLearner``).

The reference script watches training through three host-side accounts of stable_baselines3 2.3.2,
restated here from SB3's published code (SB3 is not a dependency, nothing is pinned against an SB3
run):

* ``evaluation.py::evaluate_policy``: per step ``current_rewards += rewards`` (float64),
  ``current_lengths += 1`` and a ``for i in range(n_envs)`` loop that appends a finished env's episode
  to ``episode_rewards`` / ``episode_lengths`` while ``episode_counts[i] < episode_count_targets[i]``,
  with targets ``[(n_eval_episodes + i) // n_envs for i in range(n_envs)]``;
* ``callbacks.py::EvalCallback`` with ``StopTrainingOnRewardThreshold`` (learn.py:82-91);
* the Monitor window ``ep_info_buffer = deque(maxlen=100)`` behind ``rollout/ep_rew_mean`` /
  ``ep_len_mean`` (``on_policy_algorithm.py``, ``utils.safe_mean``).

``EpisodeStats`` keeps all of it on the device: one ``adrp_episode_step`` launch per ``env.step``
(csrc/episode.hip), no host read until ``summary()`` / ``episodes()``.

Deviations from SB3, all deliberate:

* ``Evaluator.on_rollout`` is offered once per rollout, not once per step, so an evaluation happens at
  the first rollout boundary after ``n_calls`` crossed a multiple of ``eval_freq``;
* ``evaluate_policy`` polls the number of episodes still owed every ``poll_every`` steps; the steps
  taken past the last owed episode record nothing, so the result does not depend on ``poll_every``;
* no ``callback`` / ``render`` / ``warn`` arguments, no Monitor-wrapper unwrapping (the envs here report
  their own rewards), ``reward_threshold`` folded into the evaluator instead of a nested callback;
* the best model is written as a ``policy.pth``-style state dict, not as an SB3 zip.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from .policy import MODES
from .utils import abi

SUMMARY_KEYS = ("n", "ep_rew_mean", "ep_rew_std", "ep_rew_min", "ep_rew_max", "ep_len_mean", "ep_len_std", "total")


def episode_count_targets(n_eval_episodes, num_envs):
    """SB3 evaluate_policy's episode_count_targets: the episodes are spread over the envs, the later
    envs take the remainder"""
    return [(int(n_eval_episodes) + i) // int(num_envs) for i in range(int(num_envs))]


class EpisodeStats:
    """Episode returns / lengths of ``num_envs`` envs, accumulated and logged on ``device``.

    ``ring=True`` keeps the last ``capacity`` episodes (SB3's Monitor window, ``stats_window_size``),
    ``ring=False`` the first ``capacity`` (an evaluation; later ones are counted as dropped).
    ``quota``: int per env, env e is logged only for its first ``quota[e]`` episodes."""

    def __init__(self, num_envs, device, capacity=100, ring=True, quota=None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.AdrpError("no HIP device visible: libadrp has no CPU fallback")
        self.E, self.C, self.ring = int(num_envs), int(capacity), bool(ring)
        if self.E < 1 or self.C < 1:
            raise ValueError("num_envs and capacity must be at least 1")
        self.device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        if self.device.type != "cuda":
            raise ValueError("EpisodeStats lives on a GPU")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=self.device)
        self.run_return, self.run_length, self.count = z(self.E, torch.float64), z(self.E, torch.int32), z(self.E, torch.int32)
        self.meta = z(4, torch.int64)
        self.log_return, self.log_length, self.log_env = z(self.C, torch.float64), z(self.C, torch.int32), z(self.C, torch.int32)
        self.quota = None
        if quota is not None:
            q = torch.as_tensor(quota, dtype=torch.int32).reshape(-1)
            if q.numel() != self.E or bool((q < 0).any()):
                raise ValueError(f"quota must hold {self.E} non-negative ints")
            self.quota = q.to(self.device)
        self._out8 = z(8, torch.float64)
        self._io = abi.AdrpEpisodeIO()
        self._io.struct_size = ctypes.sizeof(abi.AdrpEpisodeIO)
        self._io.num_envs, self._io.capacity, self._io.ring = self.E, self.C, int(self.ring)
        for k in ("quota", "run_return", "run_length", "count", "meta", "log_return", "log_length", "log_env"):
            t = getattr(self, k)
            setattr(self._io, k, None if t is None else t.data_ptr())
        self._ref = ctypes.byref(self._io)
        self.reset()

    def reset(self):
        for t in (self.run_return, self.run_length, self.count, self.meta, self.log_return, self.log_length, self.log_env):
            t.zero_()
        if self.quota is not None:
            self.meta[1:2].copy_(self.quota.sum(dtype=torch.int64).reshape(1))    # episodes still owed

    def step(self, rew, term, trunc):
        """account one env.step: rew [E] float32, term / trunc [E] bool or uint8, contiguous on this
        device (the tensors the envs return).  One launch, no host read."""
        if not (rew.is_cuda and rew.dtype == torch.float32 and rew.is_contiguous() and rew.numel() == self.E
                and rew.device == self.device):
            raise ValueError(f"rew must be a contiguous float32 tensor of {self.E} elements on {self.device}")
        for t in (term, trunc):
            if not (t.is_cuda and t.dtype in (torch.bool, torch.uint8) and t.is_contiguous() and t.numel() == self.E
                    and t.device == self.device):
                raise ValueError(f"term / trunc must be contiguous bool or uint8 tensors of {self.E} elements on {self.device}")
        rc = self.lib.adrp_episode_step(self._ref, rew.data_ptr(), term.data_ptr(), trunc.data_ptr(),
                                        _lib._raw_stream(self.device.index))
        if rc != 0:
            raise _lib.AdrpError(f"adrp_episode_step: {self.lib.adrp_last_error(None).decode()}")

    def remaining(self):
        """episodes the quotas still owe (a host read)"""
        return int(self.meta[1])

    def summary(self):
        """{n, ep_rew_mean, ep_rew_std, ep_rew_min, ep_rew_max, ep_len_mean, ep_len_std, total} as Python
        floats over the logged episodes (the one host read); NaN means on an empty log (safe_mean)"""
        with torch.cuda.device(self.device):
            rc = self.lib.adrp_episode_summary(self._ref, self._out8.data_ptr(), _lib._raw_stream(self.device.index))
        if rc != 0:
            raise _lib.AdrpError(f"adrp_episode_summary: {self.lib.adrp_last_error(None).decode()}")
        return dict(zip(SUMMARY_KEYS, self._out8.cpu().tolist()))

    def episodes(self):
        """(returns float64 [n], lengths int32 [n], envs int32 [n]) as numpy arrays in logging order (a
        ring: oldest first)"""
        total = int(self.meta[0])
        n = min(total, self.C)
        r, l, e = (t.cpu().numpy() for t in (self.log_return, self.log_length, self.log_env))
        if self.ring and total > self.C:
            k = total % self.C                  # the oldest entry's slot
            order = np.r_[k:self.C, 0:k]
            return r[order], l[order], e[order]
        return r[:n].copy(), l[:n].copy(), e[:n].copy()

    def episode_times(self, ctrl_freq):
        """sim_time of each logged episode's last step, (length - 1) / ctrl_freq (scripts/sim.py:79, 108)"""
        return (self.episodes()[1].astype(np.float64) - 1.0) / float(ctrl_freq)


def _episode_len_sec(env):
    return float(env.cfg.track.episode_len_sec if env.cfg.task == abi.TASK_RACE else env.cfg.episode_len_sec)


def _check_env(env):
    from .envs.ctrl import StateRowAviary
    from .envs.multihover import MultiHoverAviary
    if isinstance(env, StateRowAviary):
        raise ValueError(f"{type(env).__name__} never ends an episode (no reward, no termination): nothing to evaluate")
    if not env.cfg.autoreset:
        raise ValueError("evaluate_policy needs an env built with autoreset=True (finished envs start their next episode)")
    if env.NUM_DRONES != 1 and not isinstance(env, MultiHoverAviary):
        raise ValueError("one agent per env: HoverAviary, MultiRaceAviary(num_drones=1), or MultiHoverAviary "
                         "as one joint agent (per-drone agents of a multi-drone race are not evaluated)")


def evaluate_policy(policy, env, n_eval_episodes=10, deterministic=True, return_episode_rewards=False, seed=0,
                    poll_every=8, max_steps=None):
    """SB3 ``evaluate_policy`` for a ``DevicePolicy`` on an env of this package, without a host read
    per step.  Returns (mean, std) of the episode returns, or (episode_rewards, episode_lengths) as
    lists in SB3's order.  ``deterministic=False`` samples with ``policy.sample(obs, seed, step)``."""
    _lib.load()
    if not torch.cuda.is_available():
        raise _lib.AdrpError("no HIP device visible: libadrp has no CPU fallback")
    _check_env(env)
    n_eval_episodes, poll_every = int(n_eval_episodes), max(1, int(poll_every))
    if n_eval_episodes < 1:
        raise ValueError("n_eval_episodes must be at least 1")
    if not deterministic and not policy.has_critic:
        raise ValueError("sampling needs the critic blob (DevicePolicy.set_critic): log_std lives there")
    E = env.num_envs
    quota = episode_count_targets(n_eval_episodes, E)
    if max_steps is None:
        # the longest episode has len * ctrl_freq + 2 steps: the envs test step_counter / PYB_FREQ >
        # EPISODE_LEN_SEC on the counter before the step (a full HoverAviary episode measures 242 steps at 30 Hz)
        max_steps = max(quota) * (int(np.ceil(_episode_len_sec(env) * env.CTRL_FREQ)) + 2)
    stats = EpisodeStats(E, env.device, capacity=n_eval_episodes, ring=False, quota=quota)
    with torch.cuda.device(env.device):
        obs, _ = env.reset()
        # the routing of policy.rollout: a joint MultiHoverAviary agent reads the whole [E, N D] row
        joint = obs.shape[1] > 1 and policy.in_dim == obs.shape[1] * obs.shape[2]
        raw = policy.mode == MODES["raw"]
        width = policy.act_dim if raw else 4
        if joint:
            if width != obs.shape[1] * env._act_shape[-1]:
                raise ValueError("a joint policy emits NUM_DRONES * A actions")
            act = torch.empty(tuple(env._act_shape), dtype=torch.float32, device=obs.device)
        else:
            act = torch.empty(obs.shape[:-1] + (width,), dtype=torch.float32, device=obs.device)
        rows = E if joint else obs.shape[0] * obs.shape[1]
        if not deterministic:
            scratch = (torch.empty((rows, policy.act_dim), dtype=torch.float32, device=obs.device),
                       torch.empty(rows, dtype=torch.float32, device=obs.device),
                       torch.empty(rows, dtype=torch.float32, device=obs.device))
        step, left = 0, n_eval_episodes
        while left > 0:
            if step >= max_steps:
                raise RuntimeError(f"evaluate_policy: {left} of {n_eval_episodes} episodes still open after {max_steps} steps")
            x = obs.view(E, -1) if joint else obs
            if deterministic:
                policy.act(x, out=act)
            else:
                policy.sample(x, seed, step, env_act=act.view(rows, -1), action=scratch[0], value=scratch[1],
                              log_prob=scratch[2])
            obs, rew, term, trunc, _ = env.step(act)
            stats.step(rew, term, trunc)
            step += 1
            if step % poll_every == 0 or step >= max_steps:
                left = stats.remaining()
    rets, lens, _ = stats.episodes()
    if return_episode_rewards:
        return [float(r) for r in rets], [int(n) for n in lens]
    return float(np.mean(rets)), float(np.std(rets))


class Evaluator:
    """SB3's ``EvalCallback`` with ``StopTrainingOnRewardThreshold`` as ``callback_on_new_best``
    (learn.py:82-91), offered once per rollout: ``on_rollout`` returns SB3's ``continue_training``."""

    def __init__(self, eval_env, policy, n_eval_episodes=5, eval_freq=10000, reward_threshold=None, best_path=None,
                 log_path=None, deterministic=True):
        _check_env(eval_env)
        if int(eval_freq) < 1 or int(n_eval_episodes) < 1:
            raise ValueError("eval_freq and n_eval_episodes must be at least 1")
        self.eval_env, self.policy = eval_env, policy
        self.n_eval_episodes, self.eval_freq = int(n_eval_episodes), int(eval_freq)
        self.reward_threshold = None if reward_threshold is None else float(reward_threshold)
        self.best_path, self.log_path, self.deterministic = best_path, log_path, bool(deterministic)
        self.best_mean_reward = -np.inf
        self.last_mean_reward = -np.inf
        self.evaluations_timesteps, self.evaluations_results, self.evaluations_length = [], [], []
        self.n_evaluations = 0
        self._last_calls = 0

    def on_rollout(self, num_timesteps, n_calls, learner=None):
        """``n_calls``: env.step calls so far (SB3's BaseCallback.n_calls), ``num_timesteps`` = n_calls x
        the training env's num_envs.  Evaluates when n_calls crossed a multiple of eval_freq since the
        last call; returns False when training should stop."""
        n_calls = int(n_calls)
        due = n_calls // self.eval_freq > self._last_calls // self.eval_freq
        self._last_calls = n_calls
        self.evaluated = False
        if due:
            rewards, lengths = evaluate_policy(self.policy, self.eval_env, self.n_eval_episodes, self.deterministic,
                                               return_episode_rewards=True)
            self.evaluated = True
            self.n_evaluations += 1
            self.evaluations_timesteps.append(int(num_timesteps))
            self.evaluations_results.append(list(rewards))
            self.evaluations_length.append(list(lengths))
            if self.log_path is not None:
                os.makedirs(self.log_path, exist_ok=True)
                np.savez(os.path.join(self.log_path, "evaluations.npz"), timesteps=self.evaluations_timesteps,
                         results=self.evaluations_results, ep_lengths=self.evaluations_length)
            self.last_mean_reward = float(np.mean(rewards))
            self.last_mean_length = float(np.mean(lengths))
            if self.last_mean_reward > self.best_mean_reward:
                self.best_mean_reward = self.last_mean_reward
                if self.best_path is not None and learner is not None:
                    d = os.path.dirname(os.path.abspath(self.best_path))
                    os.makedirs(d, exist_ok=True)
                    torch.save({k: v.detach().cpu() for k, v in learner.state_dict().items()}, self.best_path)
        if self.reward_threshold is None:
            return True
        return bool(self.best_mean_reward < self.reward_threshold)
