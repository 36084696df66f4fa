"""MellingerControl on the GPU: E x N Crazyflie firmware controllers, one HIP launch per ``computeControl``.

Mirrors the reference surface (control/MellingerControl.py): ``reset(init_obs)``, ``computeControl`` with the
current position, roll / pitch / yaw and velocity, which returns the four motor RPMs, and the ``send*Cmd`` family of
the high-level commander.  Everything is batched over ``[E, N, ...]`` device tensors.  The controller code is the
one the fused MultiRaceAviary step kernels run at 500 Hz (csrc/race_kernel.h mellinger_compute, csrc/commander.h):
the float64 wrapper arithmetic in the controller's precision, the firmware in C float.  One call is one firmware
tick (500 Hz), whatever ``control_timestep`` says, as in the reference.

There is no command queue.  The reference's ``send*Cmd`` append to a queue that ``process_command_queue(t)``
empties right after (low_level_control, :32-57); here every ``send*Cmd`` processes its command at once, with the
commander clock the reference's command messages carry in ``args[-1]`` (so the duration of a take-off, the relative
flag of a go-to, as the reference has it) or, given ``timestep=``, with that clock.  A
command stops the planner first, as ``process_command_queue`` does: a take-off or go-to plans from the commander's
last position, and a land command finds the planner stopped and leaves the commander idle.

``target_pos`` of ``computeControl`` is, as in the reference (:202), not a target but the per-motor thrust
disturbance [E, N, 4]; ``disturbance=`` is the honest keyword for the same thing.

Outputs are persistent device buffers that the next call overwrites; ``out=rpm`` binds a caller tensor instead.
Inputs that are not torch tensors are copied to the device in the controller's dtype; a tensor must have the
controller's dtype, or be float32 for a float64 controller.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from ..commands import CMD_ARGS, COMMAND_CODE, TIME_SLOT, _SIGNATURE
from ..utils import abi
from ..utils.enums import Command, DroneModel


def check_input_shape(name, shape, num_envs, num_drones, width):
    """an input is [E, N, width] exactly"""
    full = (num_envs, num_drones, width)
    if tuple(shape) != full:
        raise ValueError(f"{name} must have shape {full}, got {tuple(shape)}")


def check_mask(mask, num_envs, num_drones):
    """None, or a numpy uint8 [E, N] from a mask of shape [E] (envs) or [E, N] (controllers), non-zero = selected"""
    if mask is None:
        return None
    m = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask) != 0
    if m.shape == (num_envs,):
        m = np.broadcast_to(m[:, None], (num_envs, num_drones))
    if m.shape != (num_envs, num_drones):
        raise ValueError(f"mask must have shape ({num_envs},) or ({num_envs}, {num_drones}), got {m.shape}")
    return np.ascontiguousarray(m, np.uint8)


def pack_command(cmd, args, num_envs, num_drones, mask=None, timestep=None):
    """One command for every controller (or those of ``mask``; the others get Command.NONE) ->
    (codes int32 [E, N], args float64 [E, N, 14]) in commands.encode_commands' packing.  Every argument is a
    scalar / vector for all controllers, or has leading dimensions [E, N].  The commander clock (slot 13) is
    ``args[-1]``, as in the reference's command messages, unless ``timestep`` gives it."""
    E, N = int(num_envs), int(num_drones)
    codes = np.full((E, N), COMMAND_CODE[cmd], np.int32)
    out = np.zeros((E, N, CMD_ARGS), np.float64)
    args = list(args)
    sig = _SIGNATURE.get(cmd, ())
    if sig and len(args) != len(sig):
        raise TypeError(f"{cmd}: expected {len(sig)} arguments, got {len(args)}")
    if not args:
        raise IndexError(f"{cmd}: the commander clock (args[-1]) is missing")
    k = 0
    for a, w in zip(args, sig):
        v = np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a, np.float64)
        if v.shape[:2] == (E, N) and v.size == E * N * w:
            v = v.reshape(E, N, w)
        elif v.size == w:
            v = v.reshape(w)
        else:
            raise ValueError(f"{cmd}: argument of shape {v.shape}, expected width {w} or ({E}, {N}, {w})")
        out[..., k:k + w] = v
        k += w
    t = args[-1] if timestep is None else timestep
    t = np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t, np.float64)
    out[..., TIME_SLOT] = t.reshape(E, N, -1)[..., -1] if t.shape[:2] == (E, N) else t.reshape(-1)[-1]
    m = check_mask(mask, E, N)
    if m is not None:
        codes[m == 0] = COMMAND_CODE[Command.NONE]
        out[m == 0] = 0.0
    return codes, out


class MellingerControl:
    """Batched counterpart of gym_pybullet_adrp.control.MellingerControl.MellingerControl."""

    FIRMWARE_FREQ = 500

    def __init__(self, drone_model: DroneModel = DroneModel.CF2X, g: float = 9.8, *, num_envs: int = 1,
                 num_drones: int = 1, device=None, precision: str = "fp64"):
        if drone_model != DroneModel.CF2X:
            raise ValueError("[ERROR] in MellingerControl.__init__(), MellingerControl requires DroneModel.CF2X")
        if precision not in ("fp32", "fp64"):
            raise ValueError("precision must be 'fp32' or 'fp64'")
        if int(num_envs) <= 0 or int(num_drones) <= 0:
            raise ValueError("num_envs and num_drones must be > 0")
        self.lib = _lib.load()
        self.DRONE_MODEL = drone_model
        self.GRAVITY = g * 0.03454          # (BaseControl; the firmware has its own constants)
        self.KF, self.KM = 3.16e-10, 7.94e-12
        self.num_envs, self.NUM_DRONES = int(num_envs), int(num_drones)
        self.rows = self.num_envs * self.NUM_DRONES
        self.real = torch.float64 if precision == "fp64" else torch.float32
        nf, ni = ctypes.c_int(), ctypes.c_int()
        self._check_rc(self.lib.adrp_mellinger_state_layout(None, ctypes.byref(nf), ctypes.byref(ni)), "adrp_mellinger_state_layout")
        self.nf, self.ni = nf.value, ni.value
        self.h = None
        device = 0 if device is None else (device.index or 0) if isinstance(device, torch.device) else int(device)
        c = ctypes.c_void_p()
        rc = self.lib.adrp_mellinger_create(self.rows, int(precision == "fp64"), device, ctypes.byref(c))
        if rc != 0:
            msg = self.lib.adrp_last_error(None).decode()
            raise (ValueError if rc == abi.ERR_INVALID else _lib.AdrpError)(f"adrp_mellinger_create: {msg}")
        self.h = c
        self.device = torch.device("cuda", device)
        self._dev_index = self.device.index
        E, N = self.num_envs, self.NUM_DRONES
        self._rpm = torch.zeros((E, N, 4), dtype=self.real, device=self.device)
        self._codes = torch.zeros((E, N), dtype=torch.int32, device=self.device)
        self._args = torch.zeros((E, N, CMD_ARGS), dtype=torch.float64, device=self.device)
        self._dist = None
        self.control_counter = 0

    # ---- plumbing ----
    def _check_rc(self, rc, what):
        if rc != 0:
            msg = self.lib.adrp_last_error(None).decode()
            raise (ValueError if rc == abi.ERR_INVALID else _lib.AdrpError)(f"{what}: {msg}")

    def _stream(self):
        return _lib._raw_stream(self._dev_index)

    def close(self):
        if getattr(self, "h", None):
            self.lib.adrp_mellinger_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _input(self, name, t, width):
        if not isinstance(t, torch.Tensor):     # numpy and sequences are copied in the controller's dtype
            t = torch.as_tensor(np.asarray(t), dtype=self.real, device=self.device)
        check_input_shape(name, t.shape, self.num_envs, self.NUM_DRONES, width)
        if t.device != self.device:
            t = t.to(self.device)
        return t.contiguous()

    def _in_precision(self, dtype):
        if dtype == self.real:
            return int(self.real == torch.float64)
        if dtype == torch.float32 and self.real == torch.float64:
            return 0
        raise ValueError(f"inputs must be {self.real} (or float32 into a float64 controller), got {dtype}")

    def _disturbance(self, target_pos, disturbance):
        if target_pos is not None and disturbance is not None:
            raise ValueError("target_pos is the disturbance slot: give target_pos or disturbance, not both")
        d = disturbance if disturbance is not None else target_pos
        if d is None:
            return None
        shape = (self.num_envs, self.NUM_DRONES, 4)
        if isinstance(d, torch.Tensor) and d.dtype == self.real and d.device == self.device and d.shape == shape and d.is_contiguous():
            return d
        d = torch.as_tensor(np.asarray(d) if not isinstance(d, torch.Tensor) else d, dtype=self.real, device=self.device)
        if tuple(d.shape) not in ((4,), (self.NUM_DRONES, 4), shape):
            raise ValueError(f"disturbance must have shape (4,), ({self.NUM_DRONES}, 4) or {shape}, got {tuple(d.shape)}")
        if self._dist is None:
            self._dist = torch.empty(shape, dtype=self.real, device=self.device)
        self._dist.copy_(d.expand(shape))
        return self._dist

    def _out(self, out):
        if out is None:
            return self._rpm
        old = self._rpm
        if out.shape != old.shape or out.dtype != old.dtype or out.device != old.device or not out.is_contiguous():
            raise ValueError(f"out: need a contiguous {old.dtype} {tuple(old.shape)} tensor on {old.device}")
        return out

    # ---- the reference's surface, batched ----
    def reset(self, init_obs, mask=None):
        """MellingerControl.reset(init_obs) of every controller, or of those selected by mask ([E] envs or [E, N]
        controllers, non-zero = reset).  init_obs: a CtrlAviary (its last observation rows are taken), a tensor of
        state rows [E, N, 20] (pos 0:3, rpy 7:10, vel 10:13) or of rows in the reference's layout [E, N, W >= 9]
        (pos 0:3, rpy 3:6, vel 6:9)."""
        rows = getattr(init_obs, "_obs", init_obs) if isinstance(getattr(init_obs, "h", None), _lib.Handle) else init_obs
        if not isinstance(rows, torch.Tensor):
            rows = torch.as_tensor(np.asarray(rows))
        if rows.dim() != 3 or tuple(rows.shape[:2]) != (self.num_envs, self.NUM_DRONES) or rows.shape[2] < 9:
            raise ValueError(f"init_obs must have shape ({self.num_envs}, {self.NUM_DRONES}, W >= 9), got {tuple(rows.shape)}")
        a, v = ((7, 10) if rows.shape[2] == 20 else (3, 6))
        m = check_mask(mask, self.num_envs, self.NUM_DRONES)
        rows = rows.to(device=self.device, dtype=self.real)
        pos, rpy, vel = rows[..., 0:3].contiguous(), rows[..., a:a + 3].contiguous(), rows[..., v:v + 3].contiguous()
        md = None if m is None else torch.from_numpy(m).to(self.device)
        self._check_rc(self.lib.adrp_mellinger_reset(self.h, _lib._p(pos), _lib._p(rpy), _lib._p(vel), _lib._p(md),
                                                     self._stream()), "adrp_mellinger_reset")
        if m is None:
            self.control_counter = 0

    def computeControl(self, control_timestep, cur_pos, cur_rpy, cur_vel, cur_ang_vel=None, target_pos=None,
                       target_rpy=None, target_vel=None, target_rpy_rates=None, *, disturbance=None, out=None):
        """cur_pos / cur_rpy / cur_vel [E, N, 3]; control_timestep, cur_ang_vel and the last three targets are
        unused, as in the reference; target_pos (or disturbance=) is the thrust disturbance [E, N, 4], [N, 4] or [4].
        Returns rpm [E, N, 4] in the controller's dtype."""
        pos, rpy, vel = self._input("cur_pos", cur_pos, 3), self._input("cur_rpy", cur_rpy, 3), self._input("cur_vel", cur_vel, 3)
        if not (pos.dtype == rpy.dtype == vel.dtype):
            raise ValueError("cur_pos, cur_rpy and cur_vel must share a dtype")
        ip = self._in_precision(pos.dtype)
        rpm = self._out(out)
        d = self._disturbance(target_pos, disturbance)
        self._check_rc(self.lib.adrp_mellinger_compute(self.h, _lib._p(pos), _lib._p(rpy), _lib._p(vel), 0, ip, _lib._p(d),
                                                       _lib._p(rpm), self._stream()), "adrp_mellinger_compute")
        self.control_counter += 1
        return rpm

    def computeControlFromState(self, control_timestep, state, disturbance=None, out=None, rpy_out=None):
        """state: a contiguous [E, N, 20] tensor of _getDroneStateVector rows (pos 0:3, rpy 7:10, vel 10:13), or a
        CtrlAviary: the kernel then reads the env's own state columns in the env's precision and takes roll / pitch /
        yaw from its quaternion (rpy_out, [E, N, 3], receives those angles)."""
        rpm = self._out(out)
        d = self._disturbance(None, disturbance)
        handle = getattr(state, "h", None)
        if isinstance(handle, _lib.Handle):
            if handle.E * handle.N != self.rows or handle.real != self.real:
                raise ValueError(f"the env has {handle.E} x {handle.N} drones in {handle.real}; the controller "
                                 f"{self.num_envs} x {self.NUM_DRONES} in {self.real}")
            if rpy_out is not None:
                check_input_shape("rpy_out", rpy_out.shape, self.num_envs, self.NUM_DRONES, 3)
                if rpy_out.dtype != self.real or rpy_out.device != self.device or not rpy_out.is_contiguous():
                    raise ValueError(f"rpy_out: need a contiguous {self.real} tensor on {self.device}")
            self._check_rc(self.lib.adrp_mellinger_compute_env(self.h, handle.h, _lib._p(d), _lib._p(rpm), _lib._p(rpy_out),
                                                           self._stream()), "adrp_mellinger_compute_env")
        else:
            if rpy_out is not None:
                raise ValueError("rpy_out needs an env (state rows carry their angles)")
            rows = self._input("state", state, 20)
            ip = self._in_precision(rows.dtype)
            base, sz = rows.data_ptr(), rows.element_size()
            self._check_rc(self.lib.adrp_mellinger_compute(self.h, ctypes.c_void_p(base), ctypes.c_void_p(base + 7 * sz),
                                                           ctypes.c_void_p(base + 10 * sz), 20, ip, _lib._p(d), _lib._p(rpm),
                                                           self._stream()), "adrp_mellinger_compute")
        self.control_counter += 1
        return rpm

    # ---- the high-level commander ----
    def command(self, codes, args):
        """One command per controller in commands.encode_commands' packing: codes int32 [E, N], args float64
        [E, N, 14] (torch or numpy); Command.NONE (0) leaves a controller untouched."""
        E, N = self.num_envs, self.NUM_DRONES
        if tuple(codes.shape) != (E, N) or tuple(args.shape) != (E, N, CMD_ARGS):
            raise ValueError(f"codes / args must have shapes ({E}, {N}) and ({E}, {N}, {CMD_ARGS}), got "
                             f"{tuple(codes.shape)} and {tuple(args.shape)}")
        for name, t, want in (("codes", codes, (torch.int32, np.int32)), ("args", args, (torch.float64, np.float64))):
            if t.dtype not in want:
                raise ValueError(f"{name} must be {want[0]}, got {t.dtype}")
        c = codes if isinstance(codes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(codes))
        a = args if isinstance(args, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(args))
        if c.device != self.device or not c.is_contiguous():
            self._codes.copy_(c)
            c = self._codes
        if a.device != self.device or not a.is_contiguous():
            self._args.copy_(a)
            a = self._args
        self._check_rc(self.lib.adrp_mellinger_command(self.h, _lib._p(c), _lib._p(a), self._stream()), "adrp_mellinger_command")

    def _send(self, cmd, args, mask, timestep=None):
        self.command(*pack_command(cmd, args, self.num_envs, self.NUM_DRONES, mask, timestep))

    # the reference hands process_command_queue the message's last argument as the commander clock (the duration of a
    # take-off, the relative flag of a go-to); timestep= gives the clock itself instead
    def sendFullStateCmd(self, pos, vel, acc, yaw, rpy_rate, timestep, mask=None):
        self._send(Command.FULLSTATE, [pos, vel, acc, yaw, rpy_rate, timestep], mask)

    def sendTakeoffCmd(self, height, duration, mask=None, timestep=None):
        self._send(Command.TAKEOFF, [height, duration], mask, timestep)

    def sendTakeoffYawCmd(self, height, duration, yaw, mask=None, timestep=None):
        self._send(Command.TAKEOFFYAW, [height, duration, yaw], mask, timestep)

    def sendTakeoffVelCmd(self, height, vel, relative, mask=None, timestep=None):
        self._send(Command.TAKEOFFVEL, [height, vel, relative], mask, timestep)

    def sendLandCmd(self, height, duration, mask=None, timestep=None):
        self._send(Command.LAND, [height, duration], mask, timestep)

    def sendLandYawCmd(self, height, duration, yaw, mask=None, timestep=None):
        self._send(Command.LANDYAW, [height, duration, yaw], mask, timestep)

    def sendLandVelCmd(self, height, vel, relative, mask=None, timestep=None):
        self._send(Command.LANDVEL, [height, vel, relative], mask, timestep)

    def sendGotoCmd(self, pos, yaw, duration_s, relative, mask=None, timestep=None):
        self._send(Command.GOTO, [pos, yaw, duration_s, relative], mask, timestep)

    def sendStopCmd(self, timestep=0.0, mask=None):
        self._send(Command.STOP, [timestep], mask)

    def notifySetpointStop(self, timestep=0.0, mask=None):
        self._send(Command.NOTIFY, [timestep], mask)

    # ---- controller state ----
    def state_field_names(self):
        """(float field names, int field names): the race state's names for its controller part"""
        f = self.lib.adrp_mellinger_state_field
        return [f(0, k).decode() for k in range(self.nf)], [f(1, k).decode() for k in range(self.ni)]

    def get_state(self):
        """(float [nf, E * N] in the controller's dtype, int32 [ni, E * N])"""
        f = torch.empty((self.nf, self.rows), dtype=self.real, device=self.device)
        i = torch.empty((self.ni, self.rows), dtype=torch.int32, device=self.device)
        self._check_rc(self.lib.adrp_mellinger_get_state(self.h, _lib._p(f), _lib._p(i), self._stream()), "adrp_mellinger_get_state")
        return f, i

    def set_state(self, f, i):
        f = torch.as_tensor(f).to(device=self.device, dtype=self.real).contiguous()
        i = torch.as_tensor(i).to(device=self.device, dtype=torch.int32).contiguous()
        if f.shape != (self.nf, self.rows) or i.shape != (self.ni, self.rows):
            raise ValueError(f"state must have shapes ({self.nf}, {self.rows}) and ({self.ni}, {self.rows}), got "
                             f"{tuple(f.shape)} and {tuple(i.shape)}")
        self._check_rc(self.lib.adrp_mellinger_set_state(self.h, _lib._p(f), _lib._p(i), self._stream()), "adrp_mellinger_set_state")

    def get_command_state(self):
        """(float32 [63, E * N], int32 [3, E * N]): the commander's state in include/adrp.h's order"""
        f = torch.empty((abi.CMD_NF, self.rows), dtype=torch.float32, device=self.device)
        i = torch.empty((abi.CMD_NI, self.rows), dtype=torch.int32, device=self.device)
        self._check_rc(self.lib.adrp_mellinger_get_command_state(self.h, _lib._p(f), _lib._p(i), self._stream()),
                       "adrp_mellinger_get_command_state")
        return f, i

    def set_command_state(self, f, i):
        f = torch.as_tensor(f).to(device=self.device, dtype=torch.float32).contiguous()
        i = torch.as_tensor(i).to(device=self.device, dtype=torch.int32).contiguous()
        if f.shape != (abi.CMD_NF, self.rows) or i.shape != (abi.CMD_NI, self.rows):
            raise ValueError(f"command state must have shapes ({abi.CMD_NF}, {self.rows}) and ({abi.CMD_NI}, {self.rows})")
        self._check_rc(self.lib.adrp_mellinger_set_command_state(self.h, _lib._p(f), _lib._p(i), self._stream()),
                       "adrp_mellinger_set_command_state")
