"""Batched race evaluation: the reference's ``scripts/sim.py::simulate(config, controller, n_runs, n_drones)``
(scripts/sim.py:18-112) for thousands of races at once.

The reference builds a ``multi-race-aviary-v0``, gives every drone its own controller
(``HardCodedController``, ``RLController``), runs ``n_runs`` episodes one after the other and returns the
episode times.  Here the runs are covered in waves of ``E = num_envs`` races on one ``MultiRaceAviary`` built
without auto-reset; run ``r = wave * E + e``.  A wave is: ``env.reset()``, fresh controllers from the reset
observation (sim.py:72-76), then per step two small launches next to the env step (csrc/sim_kernel.h):

* ``ControllerBank.predict``: the PPO actors of the policy drones (``adrp_policy_act`` on the drone's own
  observation rows, strided in place) and one ``race_controller_kernel`` launch that writes every drone's
  command row, the scripted drones' exactly as ``hardcoded.HardCodedCommander.predict`` computes it;
* ``RaceResults.step``: ``race_results_kernel`` keeps the episode's return and length and, per drone, the
  gates passed, the step it finished at and the step it was eliminated at, read from the env handle's own
  state image, and logs them when the env closes (``terminated | truncated``).

The number of open envs is read from the device every ``poll_every`` steps; steps taken past an env's close
record nothing, so the results do not depend on it.  All envs of a wave share one episode clock,
``ep_time = k / ctrl_freq`` at step ``k`` (sim.py:79).

Deviations from the reference, all deliberate: the runs are batched in waves, not sequential; the scripted
controller plans its spline on the host by default (scipy ``splprep``, one call per distinct observation row of
the wave) and with ``planner="device"`` in one launch per wave (``adrp_race_plan``, the
same FITPACK fit restated in csrc/spline_plan.h); the other reference controllers (``HoverController``, the TwoGates scripted
one) are not built; there is no GUI timer.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .commands import CMD_ARGS
from .controllers import entry_kinds, plan_commander, policies_act
from .policy import MODES, DevicePolicy
from .utils import abi
from .utils.enums import Physics, RaceMode

MAX_WAVE = 4096          # default num_envs cap of simulate()


def _need_gpu():
    _lib.load()
    if not torch.cuda.is_available():
        raise _lib.AdrpError("no HIP device visible: libadrp has no CPU fallback")


def _expand(controllers, n_drones):
    """one entry per drone, or a single entry used for all drones (scripts/sim.py:57-60)"""
    if isinstance(controllers, (str, DevicePolicy)) or controllers is None:
        controllers = [controllers]
    controllers = list(controllers)
    if len(controllers) == 1:
        controllers = controllers * int(n_drones)
    if len(controllers) != int(n_drones):
        raise ValueError(f"{len(controllers)} controllers for {int(n_drones)} drones: give one, or one per drone")
    return controllers


class ControllerBank:
    """One controller per drone of a ``MultiRaceAviary`` batch: ``"hardcoded"`` (HardCodedController, delay =
    drone index as scripts/sim.py:75), a ``DevicePolicy`` in mode "relative" / "absolute" (RLController /
    RLControllerTwoGates) or ``None`` (the drone gets Command.NONE).  ``predict`` returns the encoded
    ``(codes int32 [E, N], args float64 [E, N, 14])`` pair ``env.step`` takes; the buffers are persistent."""

    def __init__(self, env, controllers, planner="host"):
        if planner not in ("host", "device"):
            raise ValueError(f"planner must be 'host' or 'device', not {planner!r}")
        self.planner = planner
        _need_gpu()
        self.lib = _lib.load()
        self.E, self.N, self.D = int(env.num_envs), int(env.NUM_DRONES), int(env.h.D)
        self.device = env.device
        self.controllers = _expand(controllers, self.N)
        self.kinds = entry_kinds(self.controllers, self.D, self.device, "controller")
        E, N = self.E, self.N
        self.codes = torch.zeros((E, N), dtype=torch.int32, device=self.device)
        self.args = torch.zeros((E, N, CMD_ARGS), dtype=torch.float64, device=self.device)
        self.phase = torch.zeros((3, E, N), dtype=torch.uint8, device=self.device)      # took off, notified, landed
        self.setpoints = torch.zeros((N, E, 4), dtype=torch.float32, device=self.device)  # drone-major
        self.commander = None
        self._io = abi.AdrpRaceCtrlIO()
        self._io.struct_size = ctypes.sizeof(abi.AdrpRaceCtrlIO)
        self._io.num_envs, self._io.num_drones = E, N
        for n, k in enumerate(self.kinds):
            self._io.kind[n] = k
        self._io.phase, self._io.setpoints = self.phase.data_ptr(), self.setpoints.data_ptr()
        self._io.codes, self._io.args = self.codes.data_ptr(), self.args.data_ptr()
        self._ref = ctypes.byref(self._io)
        self._policies = [(n, c) for n, c in enumerate(self.controllers) if self.kinds[n] == abi.RACE_CTRL_POLICY]

    @property
    def has_hardcoded(self):
        return abi.RACE_CTRL_HARDCODED in self.kinds

    def reset(self, obs0, delay=None):
        """fresh controllers from the reset observation (scripts/sim.py:72-76): the scripted drones re-plan, every
        phase flag is cleared"""
        if self.has_hardcoded:
            self.commander = plan_commander(self.commander, self._io, obs0, self.device, self.planner, delay=delay)
        self.phase.zero_()

    def predict(self, obs, ep_time):
        """obs: the env's observation [E, N, D] (contiguous float32 on the env's device); ep_time: seconds since the
        wave's reset, one clock for all envs.  Launches only: no host read."""
        if self.has_hardcoded and self.commander is None:
            raise RuntimeError("ControllerBank.reset(obs0) first: the scripted drones plan from the reset observation")
        stream = _lib._raw_stream(self.device.index)
        if self._policies:
            if not (obs.is_cuda and obs.dtype == torch.float32 and obs.is_contiguous()
                    and tuple(obs.shape) == (self.E, self.N, self.D) and obs.device == self.device):
                raise ValueError(f"obs must be a contiguous float32 [{self.E}, {self.N}, {self.D}] tensor on {self.device}")
            policies_act(self.lib, self._policies, obs, self.setpoints, stream)
        rc = self.lib.adrp_race_controllers(self._ref, float(ep_time), stream)
        if rc != 0:
            raise _lib.AdrpError(self.lib.adrp_last_error(None).decode())
        return self.codes, self.args


class RaceResults:
    """Per-run and per-drone race outcomes of ``n_runs`` episodes, accumulated on the device in waves of
    ``num_envs`` (include/adrp.h adrp_race_results_*).  ``begin(base, n_open)`` opens a wave whose env ``e`` is
    run ``base + e``; ``step`` accounts one env.step; ``remaining()`` is the number of envs still open (a host
    read).  The host views are read once, after the run."""

    # adrp_race_results_io field -> attribute (the running per-drone arrays are run_*, ``gates`` is the host view)
    BUFFERS = {"open": "open", "run_return": "run_return", "run_length": "run_length", "gates": "run_gates",
               "finish": "run_finish", "elim": "run_elim", "meta": "meta", "log_return": "log_return",
               "log_length": "log_length", "log_term": "log_term", "log_trunc": "log_trunc", "log_gates": "log_gates",
               "log_finish": "log_finish", "log_elim": "log_elim"}

    def __init__(self, num_envs, num_drones, n_runs, device=0, ctrl_freq=25):
        _need_gpu()
        self.lib = _lib.load()
        self.E, self.N, self.C = int(num_envs), int(num_drones), int(n_runs)
        if self.E < 1 or self.C < 1 or not 1 <= self.N <= abi.MAX_DRONES:
            raise ValueError(f"num_envs and n_runs must be at least 1, num_drones in 1..{abi.MAX_DRONES}")
        self.ctrl_freq = float(ctrl_freq)
        self.device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        if self.device.type != "cuda":
            raise ValueError("RaceResults lives on a GPU")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        E, N, C = self.E, self.N, self.C
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)
        self.open, self.run_return, self.run_length = z(E, torch.uint8), z(E, torch.float64), z(E, torch.int32)
        self.run_gates, self.run_finish, self.run_elim = (z((E, N), torch.int32) for _ in range(3))
        self.meta = z(4, torch.int64)
        self.log_return, self.log_length = z(C, torch.float64), z(C, torch.int32)
        self.log_term, self.log_trunc = z(C, torch.uint8), z(C, torch.uint8)
        self.log_gates, self.log_finish, self.log_elim = (z((C, N), torch.int32) for _ in range(3))
        self.log_finish.fill_(-1)
        self.log_elim.fill_(-1)
        self._io = abi.AdrpRaceResultsIO()
        self._io.struct_size = ctypes.sizeof(abi.AdrpRaceResultsIO)
        self._io.num_envs, self._io.num_drones, self._io.capacity = E, N, C
        for field, name in self.BUFFERS.items():
            setattr(self._io, field, getattr(self, name).data_ptr())
        self._ref = ctypes.byref(self._io)
        self._host = None

    def _check(self, rc):
        if rc != 0:
            raise _lib.AdrpError(self.lib.adrp_last_error(None).decode())

    def begin(self, base, n_open):
        """open a wave: env e < n_open is run base + e"""
        self._host = None
        with torch.cuda.device(self.device):
            self._check(self.lib.adrp_race_results_begin(self._ref, int(base), int(n_open), _lib._raw_stream(self.device.index)))

    def _step_inputs(self, rew, term, trunc):
        if not (rew.is_cuda and rew.dtype == torch.float32 and rew.is_contiguous() and rew.numel() == self.E
                and rew.device == self.device):
            raise ValueError(f"rew must be a contiguous float32 tensor of {self.E} elements on {self.device}")
        for t in (term, trunc):
            if not (t.is_cuda and t.dtype in (torch.bool, torch.uint8) and t.is_contiguous() and t.numel() == self.E
                    and t.device == self.device):
                raise ValueError(f"term / trunc must be contiguous bool or uint8 tensors of {self.E} elements on {self.device}")

    def step(self, env, rew, term, trunc):
        """account one env.step of ``env`` (a MultiRaceAviary of this shape): the per-drone gate / flags are read
        from its handle's own state image, in place.  One launch, no host read."""
        self._step_inputs(rew, term, trunc)
        self._host = None
        self._check(self.lib.adrp_race_results_step_env(self._ref, env.h.h, rew.data_ptr(), term.data_ptr(), trunc.data_ptr(),
                                                        _lib._raw_stream(self.device.index)))

    def step_arrays(self, gate, flags, rew, term, trunc):
        """the same from caller tensors: gate / flags int32 [E, N] (the "gate" / "flags" rows of get_state())"""
        self._step_inputs(rew, term, trunc)
        for t in (gate, flags):
            if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == self.E * self.N
                    and t.device == self.device):
                raise ValueError(f"gate / flags must be contiguous int32 tensors of {self.E * self.N} elements on {self.device}")
        self._host = None
        self._check(self.lib.adrp_race_results_step(self._ref, gate.data_ptr(), flags.data_ptr(), rew.data_ptr(),
                                                    term.data_ptr(), trunc.data_ptr(), _lib._raw_stream(self.device.index)))

    def remaining(self):
        """envs of the current wave still open (a host read)"""
        return int(self.meta[1])

    def logged(self):
        """episodes logged so far (a host read)"""
        return int(self.meta[0])

    # ---- host views ----
    def _views(self):
        if self._host is None:
            self._host = {k: getattr(self, k).cpu().numpy() for k in self.BUFFERS.values() if k.startswith("log_")}
        return self._host

    @property
    def episode_lengths(self):
        return self._views()["log_length"]

    @property
    def episode_times(self):
        """sim_time of each run's last step, (length - 1) / ctrl_freq (scripts/sim.py:79, 108;
        EpisodeStats.episode_times' definition)"""
        return (self.episode_lengths.astype(np.float64) - 1.0) / self.ctrl_freq

    @property
    def episode_rewards(self):
        return self._views()["log_return"]

    @property
    def terminated(self):
        return self._views()["log_term"].astype(bool)

    @property
    def truncated(self):
        return self._views()["log_trunc"].astype(bool)

    @property
    def gates(self):
        """[n_runs, N] gates each drone had passed when its run closed"""
        return self._views()["log_gates"]

    @property
    def finish_step(self):
        """[n_runs, N] step (1-based, = the episode length then) the drone finished at, -1 = never"""
        return self._views()["log_finish"]

    @property
    def elim_step(self):
        """[n_runs, N] step the drone was eliminated at, -1 = never"""
        return self._views()["log_elim"]

    @property
    def finish_times(self):
        """[n_runs, N] sim_time of the finishing step, NaN where the drone did not finish"""
        f = self.finish_step
        return np.where(f >= 0, (f.astype(np.float64) - 1.0) / self.ctrl_freq, np.nan)

    @property
    def winner(self):
        """[n_runs] the drone with the smallest finish_step (ties to the lower index), -1 if nobody finished"""
        return winner_of(self.finish_step)


def winner_of(finish_step):
    f = np.asarray(finish_step)
    key = np.where(f >= 0, f, np.iinfo(np.int32).max).astype(np.int64)
    w = key.argmin(axis=1)                    # the first minimum: ties to the lower index
    return np.where((f >= 0).any(axis=1), w, -1).astype(np.int64)


def _resolve(c, device):
    """simulate()'s controller entries: 'hardcoded', 'none' / None, a DevicePolicy, or 'zip:PATH[:mode]'
    (an SB3 zip; mode 'relative', the RLController's, by default)"""
    if isinstance(c, str) and c.lower().startswith("zip:"):
        path, _, mode = c[4:].partition(":")
        if mode in MODES and mode != "raw":
            return DevicePolicy.from_zip(path, device=device, mode=mode)
        return DevicePolicy.from_zip(c[4:], device=device, mode="relative")
    return c


def simulate(config="level0", controller=("hardcoded",), n_runs=10, n_drones=2, gui=False, num_envs=None,
             racemode=RaceMode.COMPARE, precision="fp64", physics=Physics.PYB, seed=0, reward="env", obs_wrapper=0,
             poll_every=16, max_steps=None, return_results=False, device=0, planner="host"):
    """Evaluate the drones' controllers over ``n_runs`` races (scripts/sim.py::simulate): returns the list of
    episode times in run order, or the ``RaceResults`` with ``return_results=True``.

    ``controller``: one entry per drone or a single entry for all of them, each "hardcoded", a ``DevicePolicy``
    (mode "relative" / "absolute"), "zip:PATH" (an SB3 zip, loaded as a relative-mode policy) or None.
    ``num_envs``: races per wave, ``min(n_runs, 4096)`` by default.  ``max_steps`` bounds one wave.
    ``planner``: where the "hardcoded" drones plan their splines at every wave's reset: "host" (scipy, one call
    per distinct start) or "device" (one ``adrp_race_plan`` launch on the reset observation in place)."""
    from .envs.race import MultiRaceAviary
    if gui:
        raise ValueError("GUI / video recording are out of scope (DESIGN.md)")
    if planner not in ("host", "device"):
        raise ValueError(f"planner must be 'host' or 'device', not {planner!r}")
    n_runs, n_drones, poll_every = int(n_runs), int(n_drones), max(1, int(poll_every))
    if n_runs < 1:
        raise ValueError("n_runs must be at least 1")
    controllers = _expand(controller, n_drones)
    E = min(n_runs, MAX_WAVE) if num_envs is None else int(num_envs)
    if E < 1:
        raise ValueError("num_envs must be at least 1")
    _need_gpu()
    controllers = [_resolve(c, device) for c in controllers]
    env = MultiRaceAviary(config, num_drones=n_drones, physics=physics, racemode=racemode, num_envs=E, device=device,
                          precision=precision, seed=seed, autoreset=False, reward=reward, commands=True)
    try:
        if obs_wrapper:
            env.set_wrappers(reward == "wrapper", int(obs_wrapper))
        if max_steps is None:
            # the longest episode has len * ctrl_freq + 2 steps (evaluation.evaluate_policy)
            max_steps = int(np.ceil(float(env.cfg.track.episode_len_sec) * env.CTRL_FREQ)) + 2
        bank = ControllerBank(env, controllers, planner=planner)
        res = RaceResults(E, n_drones, n_runs, env.device, env.CTRL_FREQ)
        with torch.cuda.device(env.device):
            for base in range(0, n_runs, E):
                n_open = min(E, n_runs - base)
                obs, _ = env.reset()
                bank.reset(obs)
                res.begin(base, n_open)
                k, left = 0, n_open
                while left > 0:
                    if k >= max_steps:
                        raise RuntimeError(f"simulate: {left} of {n_open} races still open after {max_steps} steps")
                    obs, rew, term, trunc, _ = env.step(bank.predict(obs, k / env.CTRL_FREQ))
                    res.step(env, rew, term, trunc)
                    k += 1
                    if k % poll_every == 0 or k >= max_steps:
                        left = res.remaining()
            res._views()
    finally:
        env.close()
    return res if return_results else [float(t) for t in res.episode_times]
