"""Per-drone controller entries of a multi-drone race: what ``sim.ControllerBank`` (the race evaluation) and
``rollout.RosterRolloutCollector`` (the opponents of a PPO rollout) do alike with their list of one entry per drone.

* ``entry_kinds`` turns the entries (``"hardcoded"``, a ``DevicePolicy``, ``None``; for a roster also ``"learner"``)
  into kinds.  ``abi.RACE_CTRL_*`` and the first three ``abi.ROSTER_*`` are the same numbers (csrc/roster_kernel.h
  relies on it), so one list serves ``adrp_race_ctrl_io.kind`` and ``adrp_race_roster_io.role``.
* ``plan_commander`` makes or re-plans the scripted drones' ``HardCodedCommander`` and binds its reference table
  into the io struct.
* ``policies_act`` runs the frozen policies' actors on their drones' observation rows, in place.
"""
import torch

from . import _lib
from .policy import MODES, DevicePolicy
from .utils import abi


def entry_kinds(entries, D, device, noun, learner=False):
    """the kind of every drone's entry, [N] ints; D, device: a drone's observation row and the env's device, which a
    ``DevicePolicy`` entry has to fit; noun: what the caller calls an entry, for the refusal of an unknown one;
    learner: ``"learner"`` is an entry too (``abi.ROSTER_LEARNER``)"""
    kinds = []
    for n, c in enumerate(entries):
        if c is None or (isinstance(c, str) and c.lower() == "none"):
            kinds.append(abi.RACE_CTRL_NONE)
        elif isinstance(c, str) and c.lower() == "hardcoded":
            kinds.append(abi.RACE_CTRL_HARDCODED)
        elif learner and isinstance(c, str) and c.lower() == "learner":
            kinds.append(abi.ROSTER_LEARNER)
        elif isinstance(c, DevicePolicy):
            if c.mode == MODES["raw"] or c.act_dim != 4:
                raise ValueError(f"drone {n}: a race policy emits a setpoint (mode 'relative' or 'absolute', 4 outputs)")
            if c.in_dim > D:
                raise ValueError(f"drone {n}: the policy reads {c.in_dim} inputs, a drone's observation row has {D}")
            if c.device != device:
                raise ValueError(f"drone {n}: the policy lives on {c.device}, the env on {device}")
            kinds.append(abi.RACE_CTRL_POLICY)
        else:
            names = "'learner', 'hardcoded'" if learner else "'hardcoded'"
            raise ValueError(f"drone {n}: not a {noun}: {c!r} ({names}, a DevicePolicy or None)")
    return kinds


def plan_commander(commander, io, obs0, device, planner, delay=None):
    """the scripted drones' commander from the reset observation obs0: the first call (commander None) makes it and
    writes its reference table into io (an ``AdrpRaceCtrlIO`` or ``AdrpRaceRosterIO``: ref_len, ref, offset), a later
    one re-plans in place.  Returns the commander."""
    if commander is not None:
        commander.replan(obs0)
        return commander
    from .hardcoded import HardCodedCommander
    commander = HardCodedCommander(obs0, delay=delay, device=device, planner=planner)
    ref, off = commander.reference_trajectory, commander._offset
    assert off.dtype == torch.int64 and off.is_contiguous() and ref.is_contiguous()
    io.ref_len, io.ref, io.offset = commander.L, ref.data_ptr(), off.data_ptr()
    return commander


def policies_act(lib, policies, obs, setpoints, stream):
    """one ``adrp_policy_act`` launch per (n, policy): the actor on drone n's rows of obs [E, N, D] (contiguous
    float32), its setpoints into setpoints[n] ([N, E, 4], drone-major)"""
    E, N, D = obs.shape
    for n, p in policies:
        # drone n's rows in place: row e at obs + (e * N + n) * D, so base + n * D with stride N * D
        rc = lib.adrp_policy_act(p.h, obs.data_ptr() + 4 * n * D, E, N * D, p.mode, setpoints[n].data_ptr(), stream)
        if rc != 0:
            raise _lib.AdrpError(f"adrp_policy_act: {lib.adrp_last_error(None).decode()}")
