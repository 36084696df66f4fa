"""On-device PPO rollout collection (the consumer side of the hot path).

The reference trains with stable-baselines3 PPO (examples/learn.py:72-94): every rollout step,
``OnPolicyAlgorithm.collect_rollouts`` (stable_baselines3 2.3.2) runs ``policy(obs)`` on the host
batch, clips the actions, steps the VecEnv, bootstraps the value of time-limit truncations into the
reward, and appends (obs, action, reward, episode_start, value, log_prob) to its RolloutBuffer;
``compute_returns_and_advantage`` then runs GAE.  ``RolloutCollector`` does the same with every
tensor resident on the GPU:

* one ``adrp_policy_sample`` launch per step (actor + critic on f32 MFMA, the Gaussian sample, its
  log-probability and the clipped / RLController-transformed env action), written straight into
  the buffer row of the step;
* the env step's reward / flags are copied into the buffer row (device-to-device);
* the truncation bootstrap ``reward += gamma * V(terminal_obs)`` for envs whose episode hit the
  time limit (and not a termination), SB3 collect_rollouts;
* ``adrp_gae`` for the advantages and returns.

One agent per env: HoverAviary (learn.py's task), a one-drone MultiRaceAviary (the RLController
setting), or MultiHoverAviary (learn.py --multiagent true) as the one joint agent SB3's MlpPolicy
makes of it: the (N, D) observation flattened to N D inputs, N A outputs reshaped row-major to
(N, A), one reward / done per env.  ``collect`` can be captured in one HIP graph (every pointer is
fixed per step).

``MultiAgentRolloutCollector`` is the per-drone counterpart for a multi-drone race: every drone of a
``MultiRaceAviary(autoreset=False)`` is an agent of one shared policy, E N buffer columns, with the
per-agent bookkeeping (the RewardWrapper per drone, a drone's own episode end while its env goes on, the
validity of a dead drone's samples, the bootstrap, the episode starts) in one ``adrp_race_agents_step``
launch per step (csrc/agents_kernel.h).
"""
import ctypes

import torch

from . import _lib
from .envs.multihover import MultiHoverAviary
from .envs.race import MultiRaceAviary
from .utils import abi


class RolloutCollector:
    """``n_steps`` x ``num_envs`` PPO rollout buffer on the env's device.

    policy: ``DevicePolicy`` with a critic (``set_critic`` / ``from_zip(critic=True)``), its input
    the first ``policy.in_dim`` obs floats of the agent's row; for MultiHoverAviary the whole joint
    row (``in_dim == NUM_DRONES * D``, ``act_dim == NUM_DRONES * A``, raw mode).

    episode_stats: an ``evaluation.EpisodeStats`` of ``num_envs`` envs (SB3's Monitor window behind
    rollout/ep_rew_mean / ep_len_mean): every step's env reward and flags are accounted there, before
    the time-limit bootstrap is added to the stored reward.  None: ``collect`` launches what it always did."""

    def __init__(self, env, policy, n_steps, gamma=0.99, gae_lambda=0.95, seed=0, episode_stats=None):
        if not policy.has_critic:
            raise ValueError("the policy needs a critic (DevicePolicy.set_critic) to collect rollouts")
        N = env.NUM_DRONES
        if N != 1 and not isinstance(env, MultiHoverAviary):
            raise ValueError("one agent per env: HoverAviary, MultiRaceAviary(num_drones=1), or MultiHoverAviary "
                             "as one joint agent (per-drone agents of a multi-drone race are not collected)")
        # the agent's row: all N drones' rows side by side (SB3 flattens the (N, D) observation)
        D, A = N * env.h.D, policy.act_dim
        if N != 1:
            if policy.in_dim != D:
                raise ValueError(f"a joint MultiHoverAviary policy reads NUM_DRONES * D = {D} inputs, not {policy.in_dim}")
            if policy.mode != 0 or A != N * env.h.A:
                raise ValueError(f"a joint MultiHoverAviary policy emits NUM_DRONES * A = {N * env.h.A} raw actions")
        elif policy.in_dim > D:
            raise ValueError(f"the policy reads {policy.in_dim} inputs, the env's rows have {D}")
        if episode_stats is not None and (episode_stats.E != env.num_envs or episode_stats.device != env.device):
            raise ValueError("episode_stats must hold num_envs envs on the env's device")
        self.env, self.policy, self.episode_stats = env, policy, episode_stats
        self.T, self.E = int(n_steps), env.num_envs
        self.gamma, self.gae_lambda, self.seed = float(gamma), float(gae_lambda), int(seed)
        dev = env.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.obs = torch.zeros((self.T, self.E, D), **f32)
        self.actions = torch.zeros((self.T, self.E, A), **f32)
        self.rewards = torch.zeros((self.T, self.E), **f32)
        self.episode_starts = torch.zeros((self.T, self.E), **f32)
        self.values = torch.zeros((self.T, self.E), **f32)
        self.log_probs = torch.zeros((self.T, self.E), **f32)
        self.advantages = torch.zeros((self.T, self.E), **f32)
        self.returns = torch.zeros((self.T, self.E), **f32)
        self._env_act = torch.zeros((self.E,) + tuple(env._act_shape[1:]), **f32)
        self._term = torch.zeros((self.T, self.E), dtype=torch.bool, device=dev)
        self._trunc = torch.zeros((self.T, self.E), dtype=torch.bool, device=dev)
        self._last_obs = torch.zeros((self.E, D), **f32)
        self._last_start = torch.ones(self.E, **f32)         # SB3: _last_episode_starts = ones at reset
        self.last_values = torch.zeros(self.E, **f32)
        self.last_dones = torch.zeros(self.E, **f32)
        # value of the terminal observations (scratch outputs of the sampling launch)
        self._tv = torch.zeros(self.E, **f32)
        self._scratch = (torch.zeros((self.E, 4 if policy.mode else A), **f32), torch.zeros((self.E, A), **f32),
                         torch.zeros(self.E, **f32))
        self.rollouts = 0

    def reset(self):
        obs, _ = self.env.reset()
        self._last_obs.copy_(obs.reshape(self.E, -1))
        self._last_start.fill_(1.0)

    def _values_of(self, obs2d, out):
        """critic values of obs rows (the sampling launch; its action outputs go to scratch)"""
        ea, a, lp = self._scratch
        self.policy.sample(obs2d, self.seed, 0xFFFFFFFF, env_act=ea, action=a, value=out, log_prob=lp)

    def collect(self):
        """one rollout of n_steps env.steps -> fills the buffer and runs GAE (SB3 collect_rollouts +
        compute_returns_and_advantage); every tensor stays on the device"""
        # the env's device is the current one for the whole rollout: the launches take that device's
        # current stream (a null stream is the current device's)
        with torch.cuda.device(self.obs.device):
            return self._collect()

    def _collect(self):
        env, pol, E, meter = self.env, self.policy, self.E, self.episode_stats
        base = self.rollouts * self.T
        env_act = self._env_act.view(E, -1)
        for t in range(self.T):
            self.obs[t].copy_(self._last_obs)
            self.episode_starts[t].copy_(self._last_start)
            pol.sample(self.obs[t], self.seed, base + t, env_act=env_act, action=self.actions[t],
                       value=self.values[t], log_prob=self.log_probs[t])
            obs, rew, term, trunc, info = env.step(self._env_act)
            self.rewards[t].copy_(rew)
            self._term[t].copy_(term)
            self._trunc[t].copy_(trunc)
            if meter is not None:
                meter.step(rew, term, trunc)      # the env's own reward (Monitor sits below the bootstrap)
            # time-limit bootstrap (collect_rollouts): reward += gamma * V(terminal obs) only where the
            # episode was truncated and not terminated; a select, so a stale terminal row of an env
            # that did not finish (even a non-finite one) never reaches its reward
            self._values_of(info["terminal_observation"].reshape(E, -1), self._tv)
            boot = trunc & ~term
            torch.where(boot, self.rewards[t] + self.gamma * self._tv, self.rewards[t], out=self.rewards[t])
            self._last_obs.copy_(obs.reshape(E, -1))
            self._last_start.copy_((term | trunc).to(torch.float32))
        # values of the observations after the last step (SB3: policy.predict_values(new_obs))
        self._values_of(self._last_obs, self.last_values)
        self.last_dones.copy_(self._last_start)
        rc = _lib.load().adrp_gae(self.rewards.data_ptr(), self.values.data_ptr(), self.episode_starts.data_ptr(),
                                  self.last_values.data_ptr(), self.last_dones.data_ptr(), self.T, E, self.gamma,
                                  self.gae_lambda, self.advantages.data_ptr(), self.returns.data_ptr(),
                                  _lib._raw_stream(self.obs.device.index))
        if rc != 0:
            raise _lib.AdrpError(f"adrp_gae: {_lib.load().adrp_last_error(None).decode()}")
        self.rollouts += 1
        return self

    def batches(self, batch_size, generator=None):
        """RolloutBuffer.get(batch_size): shuffled minibatches of (obs, actions, old_values,
        old_log_prob, advantages, returns) over the flattened n_steps x num_envs samples"""
        n = self.T * self.E
        idx = torch.randperm(n, device=self.obs.device, generator=generator)
        flat = (self.obs.reshape(n, -1), self.actions.reshape(n, -1), self.values.reshape(n),
                self.log_probs.reshape(n), self.advantages.reshape(n), self.returns.reshape(n))
        for s in range(0, n, batch_size):
            j = idx[s:s + batch_size]
            yield tuple(x.index_select(0, j) for x in flat)


class MultiAgentRolloutCollector:
    """``n_steps`` x (``num_envs`` x ``NUM_DRONES``) PPO rollout buffer of a multi-drone race: column
    ``e * N + n`` is drone n of env e, every drone an agent of the one shared ``policy`` (its input the first
    ``policy.in_dim`` floats of the drone's own obs row, four outputs: the FULLSTATE setpoint).

    The env must not auto-reset: a drone that is eliminated or finishes ends its own agent episode while the
    env goes on, and from then until the env's reset its samples are not valid (``valid`` [T, E N] uint8; reward
    0, ``episode_starts`` 1).  The collector resets the envs that terminated or were truncated itself, by the
    device mask.  The reward is utils/wrapper.py's RewardWrapper per drone (the env's own ``reward=`` setting is
    not read).  ``T``, ``E`` (= E N: what ``PPOLearner`` sees as columns) and the flat buffers are
    ``RolloutCollector``'s; ``collect`` makes no host read.

    A dead drone's slots stay in the buffers: the policy is still sampled on whatever row the env emits for it,
    its env action is sent, and its value is stored.  ``adrp_gae`` multiplies the next value by ``1 - start``
    (a product, not a select), so the last valid sample of an agent needs the critic's value of the dead drone's
    next row to be finite: the env keeps emitting finite rows for eliminated and finished drones.  An env that
    did not would need the dead rows' values zeroed before GAE (deviation 2)."""

    def __init__(self, env, policy, n_steps, gamma=0.99, gae_lambda=0.95, seed=0):
        if not isinstance(env, MultiRaceAviary):
            raise ValueError("per-drone agents are collected from a MultiRaceAviary")
        if env.cfg.autoreset:
            raise ValueError("per-drone agents need MultiRaceAviary(autoreset=False): the collector resets the finished "
                             "envs itself, after the agents' step")
        if not policy.has_critic:
            raise ValueError("the policy needs a critic (DevicePolicy.set_critic) to collect rollouts")
        D, A = env.h.D, policy.act_dim
        if A != 4:
            raise ValueError("a race agent's policy emits the 4 FULLSTATE outputs (x, y, z, yaw)")
        if policy.in_dim > D:
            raise ValueError(f"the policy reads {policy.in_dim} inputs, the env's rows have {D}")
        self.env, self.policy = env, policy
        self.num_envs, self.N = env.num_envs, env.NUM_DRONES
        self.T, self.E = int(n_steps), self.num_envs * self.N
        self.gamma, self.gae_lambda, self.seed = float(gamma), float(gae_lambda), int(seed)
        dev = env.device
        T, R = self.T, self.E
        f32 = dict(dtype=torch.float32, device=dev)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.obs = torch.zeros((T, R, D), **f32)
        self.actions = torch.zeros((T, R, A), **f32)
        self.rewards, self.episode_starts, self.values, self.log_probs, self.advantages, self.returns = \
            (torch.zeros((T, R), **f32) for _ in range(6))
        self.valid = z((T, R), torch.uint8)
        self.ep_return, self.ep_length = z((T, R), torch.float64), z((T, R), torch.int32)
        self._env_act = torch.zeros((self.num_envs, self.N, 4), **f32)
        self._last_obs = torch.zeros((R, D), **f32)
        self._last_start = torch.ones(R, **f32)
        self.last_values, self.last_dones, self._tv = (torch.zeros(R, **f32) for _ in range(3))
        self._scratch = (torch.zeros((R, 4), **f32), torch.zeros((R, A), **f32), torch.zeros(R, **f32))
        self._mask = z(self.num_envs, torch.bool)
        # per-agent state (adrp_race_agents_io)
        self.wr_gate, self.run_length = z(R, torch.int32), z(R, torch.int32)
        self.wr_target, self.wr_prev = z((R, 3), torch.float64), z((R, 3), torch.float64)
        self.alive, self.run_return = z(R, torch.uint8), z(R, torch.float64)
        io = abi.AdrpRaceAgentsIO()
        io.struct_size = ctypes.sizeof(abi.AdrpRaceAgentsIO)
        io.num_envs, io.num_drones, io.obs_dim, io.num_gates = self.num_envs, self.N, D, int(env.cfg.track.num_gates)
        for k in ("wr_gate", "wr_target", "wr_prev", "alive", "run_return", "run_length"):
            setattr(io, k, getattr(self, k).data_ptr())
        self._io, self._ref = io, ctypes.byref(io)
        self.lib = _lib.load()
        self.rollouts = 0

    def _check(self, rc, what):
        if rc != 0:
            raise _lib.AdrpError(f"{what}: {self.lib.adrp_last_error(None).decode()}")

    def _stream(self):
        return _lib._raw_stream(self.obs.device.index)

    def _agents_reset(self, obs, mask):
        self._check(self.lib.adrp_race_agents_reset(self._ref, obs.data_ptr(), None if mask is None else mask.data_ptr(),
                                                    self._stream()), "adrp_race_agents_reset")

    def reset(self):
        with torch.cuda.device(self.obs.device):
            obs, _ = self.env.reset()
            self._agents_reset(obs, None)
            self._last_obs.copy_(obs.view(self.E, -1))
            self._last_start.fill_(1.0)

    def _values_of(self, obs2d, out):
        """critic values of obs rows (the sampling launch; its action outputs go to scratch)"""
        ea, a, lp = self._scratch
        self.policy.sample(obs2d, self.seed, 0xFFFFFFFF, env_act=ea, action=a, value=out, log_prob=lp)

    def collect(self):
        """one rollout of n_steps env.steps -> fills the buffer and runs GAE over the E N agent columns; every
        tensor stays on the device"""
        with torch.cuda.device(self.obs.device):
            return self._collect()

    def _collect(self):
        env, pol, R = self.env, self.policy, self.E
        base = self.rollouts * self.T
        env_act = self._env_act.view(R, 4)
        step_env = self.lib.adrp_race_agents_step_env
        for t in range(self.T):
            self.obs[t].copy_(self._last_obs)
            self.episode_starts[t].copy_(self._last_start)
            pol.sample(self.obs[t], self.seed, base + t, env_act=env_act, action=self.actions[t],
                       value=self.values[t], log_prob=self.log_probs[t])
            obs, _, term, trunc, _ = env.step(self._env_act)
            # the bootstrap values: the critic on the post-step rows (read only where an alive drone's env
            # hit the time limit)
            self._values_of(obs.view(R, -1), self._tv)
            self._check(step_env(self._ref, env.h.h, obs.data_ptr(), term.data_ptr(), trunc.data_ptr(), self._tv.data_ptr(),
                                 self.gamma, self.rewards[t].data_ptr(), self.valid[t].data_ptr(),
                                 self._last_start.data_ptr(), self.ep_return[t].data_ptr(), self.ep_length[t].data_ptr(),
                                 self._stream()), "adrp_race_agents_step_env")
            torch.bitwise_or(term, trunc, out=self._mask)
            mask = self._mask.view(torch.uint8)
            obs, _ = env.reset(mask=mask)
            self._agents_reset(obs, mask)
            self._last_obs.copy_(obs.view(R, -1))
        self._values_of(self._last_obs, self.last_values)
        self.last_dones.copy_(self._last_start)
        rc = self.lib.adrp_gae(self.rewards.data_ptr(), self.values.data_ptr(), self.episode_starts.data_ptr(),
                               self.last_values.data_ptr(), self.last_dones.data_ptr(), self.T, R, self.gamma,
                               self.gae_lambda, self.advantages.data_ptr(), self.returns.data_ptr(), self._stream())
        self._check(rc, "adrp_gae")
        self.rollouts += 1
        return self

    def episode_summary(self):
        """{"ep_rew_mean", "ep_len_mean", "episodes"} of the agent episodes that ended during the last rollout
        (raw rewards, without the bootstrap): one host read, after the rollout; NaN means without an episode"""
        ended = self.ep_length > 0
        n = ended.sum()
        ret = torch.where(ended, self.ep_return, torch.zeros_like(self.ep_return)).sum()
        out = torch.stack((n.double(), ret, self.ep_length.sum().double())).cpu().tolist()
        k = int(out[0])
        return {"ep_rew_mean": out[1] / k if k else float("nan"), "ep_len_mean": out[2] / k if k else float("nan"),
                "episodes": k}
