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

``RosterRolloutCollector`` adds opponents to it: a roster gives every drone a role (the learner, the scripted
``HardCodedController``, a frozen policy, none), only the learner drones have buffer columns, and every drone is
driven through the env's command path on its own env's episode clock (csrc/roster_kernel.h).

The three are three classes with their own column layouts and step sequences.  What they have in common stands
once: ``_Collector`` owns the ``n_steps`` x columns buffers, the sampling head of a step, and the tail of a rollout
(the last values, ``adrp_gae``); ``_RaceAgentsCollector`` on top of it is the race part of the two per-drone
collectors (their refusals, the validity and episode buffers, the ``adrp_race_agents_io`` over every drone slot).
A roster's entries are parsed by ``controllers.entry_kinds``, which ``sim.ControllerBank`` shares.
"""
import ctypes

import torch

from . import _lib
from .controllers import entry_kinds, plan_commander, policies_act
from .envs.multihover import MultiHoverAviary
from .envs.race import MultiRaceAviary
from .policy import MODES
from .utils import abi


class _Collector:
    """The ``n_steps`` x ``columns`` buffers of a collector (``T``, ``E``; one column per agent, ``D`` observation
    floats each), the two pieces of ``_collect`` that do not depend on the column layout (``_sample_row``,
    ``_finish``), and the plumbing around the library."""

    def __init__(self, env, policy, n_steps, columns, D, gamma, gae_lambda, seed):
        self.env, self.policy = env, policy
        self.T, self.E = int(n_steps), int(columns)
        self.gamma, self.gae_lambda, self.seed = float(gamma), float(gae_lambda), int(seed)
        T, R, A = self.T, self.E, policy.act_dim
        f32 = dict(dtype=torch.float32, device=env.device)
        self.obs = torch.zeros((T, R, D), **f32)
        self.actions = torch.zeros((T, R, A), **f32)
        self.rewards, self.episode_starts, self.values, self.log_probs, self.advantages, self.returns = \
            (torch.zeros((T, R), **f32) for _ in range(6))
        self._last_start = torch.ones(R, **f32)         # SB3: _last_episode_starts = ones at reset
        # _tv: value of the terminal observations; _scratch: the other outputs of a sampling launch made for its values
        self.last_values, self.last_dones, self._tv = (torch.zeros(R, **f32) for _ in range(3))
        self._scratch = (torch.zeros((R, 4 if policy.mode else A), **f32), torch.zeros((R, A), **f32), torch.zeros(R, **f32))
        self.lib = _lib.load()
        self.rollouts = 0

    def _check(self, rc, what):
        if rc != 0:
            raise _lib.AdrpError(f"{what}: {self.lib.adrp_last_error(None).decode()}")

    def _stream(self):
        return _lib._raw_stream(self.obs.device.index)

    def _values_of(self, obs2d, out):
        """critic values of obs rows (the sampling launch; its action outputs go to scratch)"""
        ea, a, lp = self._scratch
        self.policy.sample(obs2d, self.seed, 0xFFFFFFFF, env_act=ea, action=a, value=out, log_prob=lp)

    def collect(self):
        """one rollout of n_steps env.steps -> fills the buffer and runs GAE over its columns (SB3 collect_rollouts +
        compute_returns_and_advantage); every tensor stays on the device"""
        # the env's device is the current one for the whole rollout: the launches take that device's
        # current stream (a null stream is the current device's)
        with torch.cuda.device(self.obs.device):
            return self._collect()

    def _sample_row(self, t, counter, env_act):
        """the head of step t, once ``obs[t]`` is filled: the episode starts, and the policy sampled on the row (draw
        ``counter``) into the buffer rows of t and into env_act"""
        self.episode_starts[t].copy_(self._last_start)
        self.policy.sample(self.obs[t], self.seed, counter, env_act=env_act, action=self.actions[t],
                           value=self.values[t], log_prob=self.log_probs[t])

    def _finish(self, last_obs):
        """the tail of a rollout: values of the observations after the last step (SB3: policy.predict_values(new_obs)),
        the last dones, GAE"""
        self._values_of(last_obs, self.last_values)
        self.last_dones.copy_(self._last_start)
        rc = self.lib.adrp_gae(self.rewards.data_ptr(), self.values.data_ptr(), self.episode_starts.data_ptr(),
                               self.last_values.data_ptr(), self.last_dones.data_ptr(), self.T, self.E, self.gamma,
                               self.gae_lambda, self.advantages.data_ptr(), self.returns.data_ptr(), self._stream())
        self._check(rc, "adrp_gae")
        self.rollouts += 1
        return self

    def batches(self, batch_size, generator=None):
        """RolloutBuffer.get(batch_size): shuffled minibatches of (obs, actions, old_values,
        old_log_prob, advantages, returns) over the flattened n_steps x columns samples"""
        n = self.T * self.E
        idx = torch.randperm(n, device=self.obs.device, generator=generator)
        flat = (self.obs.reshape(n, -1), self.actions.reshape(n, -1), self.values.reshape(n),
                self.log_probs.reshape(n), self.advantages.reshape(n), self.returns.reshape(n))
        for s in range(0, n, batch_size):
            j = idx[s:s + batch_size]
            yield tuple(x.index_select(0, j) for x in flat)


class RolloutCollector(_Collector):
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
        super().__init__(env, policy, n_steps, env.num_envs, D, gamma, gae_lambda, seed)
        self.episode_stats = episode_stats
        dev = env.device
        self._env_act = torch.zeros((self.E,) + tuple(env._act_shape[1:]), dtype=torch.float32, device=dev)
        self._term = torch.zeros((self.T, self.E), dtype=torch.bool, device=dev)
        self._trunc = torch.zeros((self.T, self.E), dtype=torch.bool, device=dev)
        self._last_obs = torch.zeros((self.E, D), dtype=torch.float32, device=dev)

    def reset(self):
        obs, _ = self.env.reset()
        self._last_obs.copy_(obs.reshape(self.E, -1))
        self._last_start.fill_(1.0)

    def _collect(self):
        env, E, meter = self.env, self.E, self.episode_stats
        base = self.rollouts * self.T
        env_act = self._env_act.view(E, -1)
        for t in range(self.T):
            self.obs[t].copy_(self._last_obs)
            self._sample_row(t, base + t, env_act)
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
        return self._finish(self._last_obs)


class _RaceAgentsCollector(_Collector):
    """The race part of the two per-drone collectors, whatever their columns are: the refusals of an env or a policy
    that cannot be collected from, the validity and agent-episode buffers of the columns, and the per-agent state of
    all ``num_envs * N`` drone slots behind an ``adrp_race_agents_io`` (csrc/agents_kernel.h)."""

    @staticmethod
    def _refuse_env(env, who_is, who_needs):
        if not isinstance(env, MultiRaceAviary):
            raise ValueError(f"{who_is} collected from a MultiRaceAviary")
        if env.cfg.autoreset:
            raise ValueError(f"{who_needs} MultiRaceAviary(autoreset=False): the collector resets the finished envs "
                             "itself, after the agents' step")

    @staticmethod
    def _refuse_policy(policy, D):
        if not policy.has_critic:
            raise ValueError("the policy needs a critic (DevicePolicy.set_critic) to collect rollouts")
        if policy.act_dim != 4:
            raise ValueError("a race agent's policy emits the 4 FULLSTATE outputs (x, y, z, yaw)")
        if policy.in_dim > D:
            raise ValueError(f"the policy reads {policy.in_dim} inputs, the env's rows have {D}")

    def __init__(self, env, policy, n_steps, columns, gamma, gae_lambda, seed):
        D = env.h.D
        super().__init__(env, policy, n_steps, columns, D, gamma, gae_lambda, seed)
        self.num_envs, self.N = env.num_envs, env.NUM_DRONES
        T, R, S = self.T, self.E, self.num_envs * self.N
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=env.device)
        self.valid = z((T, R), torch.uint8)
        self.ep_return, self.ep_length = z((T, R), torch.float64), z((T, R), torch.int32)
        self._mask = z(self.num_envs, torch.bool)
        # per-agent state (adrp_race_agents_io): every drone slot, whether it has a column or not
        self.wr_gate, self.run_length = z(S, torch.int32), z(S, torch.int32)
        self.wr_target, self.wr_prev = z((S, 3), torch.float64), z((S, 3), torch.float64)
        self.alive, self.run_return = z(S, torch.uint8), z(S, torch.float64)
        io = abi.AdrpRaceAgentsIO()
        io.struct_size = ctypes.sizeof(abi.AdrpRaceAgentsIO)
        io.num_envs, io.num_drones, io.obs_dim, io.num_gates = self.num_envs, self.N, D, int(env.cfg.track.num_gates)
        for k in ("wr_gate", "wr_target", "wr_prev", "alive", "run_return", "run_length"):
            setattr(io, k, getattr(self, k).data_ptr())
        self._io, self._ref = io, ctypes.byref(io)

    def _agents_reset(self, obs, mask):
        self._check(self.lib.adrp_race_agents_reset(self._ref, obs.data_ptr(), None if mask is None else mask.data_ptr(),
                                                    self._stream()), "adrp_race_agents_reset")

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


class MultiAgentRolloutCollector(_RaceAgentsCollector):
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
        self._refuse_env(env, "per-drone agents are", "per-drone agents need")
        self._refuse_policy(policy, env.h.D)
        super().__init__(env, policy, n_steps, env.num_envs * env.NUM_DRONES, gamma, gae_lambda, seed)
        f32 = dict(dtype=torch.float32, device=env.device)
        self._env_act = torch.zeros((self.num_envs, self.N, 4), **f32)
        self._last_obs = torch.zeros((self.E, env.h.D), **f32)

    def reset(self):
        with torch.cuda.device(self.obs.device):
            obs, _ = self.env.reset()
            self._agents_reset(obs, None)
            self._last_obs.copy_(obs.view(self.E, -1))
            self._last_start.fill_(1.0)

    def _collect(self):
        env, R = self.env, self.E
        base = self.rollouts * self.T
        env_act = self._env_act.view(R, 4)
        step_env = self.lib.adrp_race_agents_step_env
        for t in range(self.T):
            self.obs[t].copy_(self._last_obs)
            self._sample_row(t, base + t, env_act)
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
        return self._finish(self._last_obs)


class RosterRolloutCollector(_RaceAgentsCollector):
    """Per-drone PPO rollouts of a multi-drone race against opponents: ``roster`` gives every drone one role,
    ``"learner"`` (a sample of ``policy``, the one being trained), ``"hardcoded"`` (the scripted
    HardCodedController, delay = drone index as ``sim.ControllerBank``), a frozen ``DevicePolicy`` in mode
    "relative" / "absolute" (e.g. ``PPOLearner.snapshot()``: self-play) or ``None`` (the drone gets Command.NONE).

    Only the L learner drones have buffer columns: ``E`` = L x num_envs, column ``l * num_envs + e`` is learner l
    (the l-th "learner" entry of the roster) in env e, drone-major.  ``T``, ``E``, the flat buffers, ``valid``,
    ``ep_return`` / ``ep_length`` and ``episode_summary()`` are ``MultiAgentRolloutCollector``'s, so
    ``PPOLearner.train(col)`` works unchanged.  The env must be a ``MultiRaceAviary(autoreset=False,
    commands=True)``: every step goes through the command path ``simulate()`` evaluates the agent under, with the
    episode time of each env's own clock.  Per step next to ``env.step``: L strided row copies, one sampling
    launch over the L E compact rows, one ``adrp_policy_act`` per frozen drone, and the three roster launches
    (csrc/roster_kernel.h).  ``collect`` makes no host read.

    The scripted drones plan once, in ``reset()``, from the reset observation (``planner``: "host" or "device");
    an env reset during a rollout restarts its scripted drones' clock and phases but does not re-plan.

    ``end_on``: "env" resets an env when its race is over (``term | trunc``), so a learner that dies early waits,
    not valid, until its opponents are done.  "learners" also resets an env once none of its learner drones has a
    running agent episode (``adrp_race_roster_done``, one more launch per step, after the learners' step): against
    a scripted racer that flies its whole spline, the rows of a rollout are then almost all valid."""

    def __init__(self, env, policy, roster, n_steps, gamma=0.99, gae_lambda=0.95, seed=0, planner="host", end_on="env"):
        if end_on not in ("env", "learners"):
            raise ValueError(f"end_on must be 'env' or 'learners', not {end_on!r}")
        self._refuse_env(env, "a roster is", "a roster needs")
        if not env.commands:
            raise ValueError("a roster needs MultiRaceAviary(commands=True): every drone is driven through the command path")
        if planner not in ("host", "device"):
            raise ValueError(f"planner must be 'host' or 'device', not {planner!r}")
        self._refuse_policy(policy, env.h.D)
        roster = list(roster)
        if len(roster) != env.NUM_DRONES:
            raise ValueError(f"the roster has {len(roster)} entries for {env.NUM_DRONES} drones: give one per drone")
        self.roles = entry_kinds(roster, env.h.D, env.device, "roster entry", learner=True)
        self.learners = [n for n, r in enumerate(self.roles) if r == abi.ROSTER_LEARNER]
        if not self.learners:
            raise ValueError("the roster has no 'learner' drone: nothing to collect")
        self._frozen = [(n, roster[n]) for n, r in enumerate(self.roles) if r == abi.ROSTER_POLICY]
        self.L = len(self.learners)
        super().__init__(env, policy, n_steps, self.L * env.num_envs, gamma, gae_lambda, seed)
        self.roster, self.planner, self.end_on = roster, planner, end_on
        R, E, N = self.E, self.num_envs, self.N
        f32 = dict(dtype=torch.float32, device=env.device)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=env.device)
        self._post = torch.zeros((R, env.h.D), **f32)               # the learner rows after the step, compact
        # the roster (adrp_race_roster_io)
        self.clock = z(E, torch.int32)
        self.phase = z((3, E, N), torch.uint8)                      # took off, notified, landed
        self.setpoints = torch.zeros((N, E, 4), **f32)              # the frozen policies', drone-major
        self.learner_act = torch.zeros((self.L, E, 4), **f32)       # the learner's env_act, drone-major
        self.codes = z((E, N), torch.int32)
        self.args = z((E, N, abi.CMD_ARGS), torch.float64)
        self.commander = None
        rio = abi.AdrpRaceRosterIO()
        rio.struct_size = ctypes.sizeof(abi.AdrpRaceRosterIO)
        rio.num_envs, rio.num_drones, rio.num_learners, rio.ctrl_freq = E, N, self.L, float(env.CTRL_FREQ)
        for n, r in enumerate(self.roles):
            rio.role[n] = r
            rio.learner_index[n] = self.learners.index(n) if r == abi.ROSTER_LEARNER else -1
        for k in ("clock", "phase", "setpoints", "learner_act", "codes", "args"):
            setattr(rio, k, getattr(self, k).data_ptr())
        self._rio, self._rref = rio, ctypes.byref(rio)

    @property
    def has_hardcoded(self):
        return abi.ROSTER_HARDCODED in self.roles

    def set_opponent(self, n, policy):
        """replace the frozen policy of drone ``n`` (a roster entry that was given as a ``DevicePolicy``), e.g. by a
        newer ``PPOLearner.snapshot()``; takes effect from the next step.  The caller closes the old one."""
        if self.roles[n] != abi.ROSTER_POLICY:
            raise ValueError(f"drone {n} is not a frozen-policy drone of this roster")
        if policy.mode == MODES["raw"] or policy.act_dim != 4 or policy.in_dim > self.env.h.D or policy.device != self.env.device:
            raise ValueError(f"drone {n}: a race policy emits a setpoint (mode 'relative' or 'absolute', 4 outputs) from a "
                             "drone's observation row, on the env's device")
        self._frozen = [(k, policy if k == n else p) for k, p in self._frozen]
        self.roster[n] = policy

    def _gather(self, dst, obs):
        """the learner drones' rows of obs [E, N, D] into the compact dst [L E, D]: one strided copy per learner"""
        rows = dst.view(self.L, self.num_envs, -1)
        for l, n in enumerate(self.learners):
            rows[l].copy_(obs[:, n])

    def _tick(self, mask):
        self._check(self.lib.adrp_race_roster_tick(self._rref, None if mask is None else mask.data_ptr(), self._stream()),
                    "adrp_race_roster_tick")

    def reset(self):
        """resets every env; the scripted drones plan their splines from this observation (the one host-side
        piece: scipy, or the device planner's status read)"""
        with torch.cuda.device(self.obs.device):
            obs, _ = self.env.reset()
            if self.has_hardcoded:
                self.commander = plan_commander(self.commander, self._rio, obs, self.env.device, self.planner)
            self._agents_reset(obs, None)
            self._tick(None)
            self._last_start.fill_(1.0)
            self._env_obs = obs

    def _collect(self):
        env, R = self.env, self.E
        if getattr(self, "_env_obs", None) is None:
            raise RuntimeError("RosterRolloutCollector.reset() first: the scripted drones plan from the reset observation")
        lib, base = self.lib, self.rollouts * self.T
        obs = self._env_obs
        env_act = self.learner_act.view(R, 4)
        cmd = (self.codes, self.args)
        for t in range(self.T):
            self._gather(self.obs[t], obs)
            self._sample_row(t, base + t, env_act)
            policies_act(lib, self._frozen, obs, self.setpoints, self._stream())
            self._check(lib.adrp_race_roster_act(self._rref, self._stream()), "adrp_race_roster_act")
            obs, _, term, trunc, _ = env.step(cmd)
            # the bootstrap values: the critic on the learner drones' post-step rows
            self._gather(self._post, obs)
            self._values_of(self._post, self._tv)
            self._check(lib.adrp_race_roster_step_env(
                self._rref, self._ref, env.h.h, obs.data_ptr(), term.data_ptr(), trunc.data_ptr(), self._tv.data_ptr(),
                self.gamma, self.rewards[t].data_ptr(), self.valid[t].data_ptr(), self._last_start.data_ptr(),
                self.ep_return[t].data_ptr(), self.ep_length[t].data_ptr(), self._stream()), "adrp_race_roster_step_env")
            mask = self._mask.view(torch.uint8)
            if self.end_on == "learners":      # the race is over, or the step above left no learner alive
                self._check(lib.adrp_race_roster_done(self._rref, self._ref, term.data_ptr(), trunc.data_ptr(), mask.data_ptr(),
                                                      self._stream()), "adrp_race_roster_done")
            else:
                torch.bitwise_or(term, trunc, out=self._mask)
            obs, _ = env.reset(mask=mask)
            self._agents_reset(obs, mask)
            self._tick(mask)
        self._env_obs = obs
        self._gather(self._post, obs)
        return self._finish(self._post)
