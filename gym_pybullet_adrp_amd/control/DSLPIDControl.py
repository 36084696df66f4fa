"""DSLPIDControl on the GPU: E x N independent PID controllers, one HIP launch per ``computeControl``.

Mirrors the reference surface (control/DSLPIDControl.py, control/BaseControl.py): the constructor takes the
drone model and ``g``; ``computeControl`` / ``computeControlFromState`` take ``control_timestep``, the
current state and the four targets and return ``(rpm, pos_e, yaw_e)``; ``setPIDCoefficients`` replaces the
gains; ``reset`` zeroes the controllers.  Everything is batched over ``[E, N, ...]`` device tensors: what the
reference computes with one object per drone (examples/pid.py:126-147) is one call here.

``state`` of ``computeControlFromState`` is a contiguous ``[E, N, 20]`` tensor of ``_getDroneStateVector``
rows (the observation of CtrlAviary / VelocityAviary) or the env itself.  Given the env, the kernel reads
position, quaternion and velocity from the env's state columns in the env's own precision: the observation
rows are float32, and the attitude D term multiplies the Euler-angle difference by about 1e6 at 48 Hz, so a
float64 loop that is to follow the reference takes this path and hands ``rpm`` to ``CtrlAviary.step``
unrounded.

Outputs are persistent device buffers that the next call overwrites (as the envs' outputs are);
``out=(rpm, pos_e, yaw_e)`` binds caller tensors instead (``pos_e`` / ``yaw_e`` may be None: not written).  Inputs
that are not torch tensors (numpy, lists) are copied to the device in the controller's dtype; a tensor must have
the controller's dtype, or be float32 for a float64 controller.  Targets broadcast from ``[3]``, ``[N, 3]`` or
``[E, N, 3]``; a contiguous ``[E, N, 3]`` device tensor of the controller's dtype is read in place.

No flight quality is claimed: DroneModel.CF2X's mixer on cf2x_IROS.urdf diverges as the reference's own
loop does; DroneModel.CF2P selects the reference's other mixer.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from ..utils import abi
from ..utils.enums import DroneModel

# what BaseControl._getURDFParameter reads for the model (control/BaseControl.py:35-39): m, kf, km of
# cf2x_IROS.urdf and cf2p.urdf
URDF_PARAMETERS = {
    DroneModel.CF2X: {"m": 0.03454, "kf": 3.16e-10, "km": 7.94e-12},
    DroneModel.CF2P: {"m": 0.027, "kf": 3.16e-10, "km": 7.94e-12},
}
MIXER_CODE = {DroneModel.CF2X: abi.DSLPID_CF2X, DroneModel.CF2P: abi.DSLPID_CF2P}
_GAINS = ("p_coeff_pos", "i_coeff_pos", "d_coeff_pos", "p_coeff_att", "i_coeff_att", "d_coeff_att")
_FIELDS = ("p_for", "i_for", "d_for", "p_tor", "i_tor", "d_tor")


def check_target_shape(name, shape, num_envs, num_drones):
    """a target broadcasts from [3], [N, 3] or [E, N, 3]"""
    full = (num_envs, num_drones, 3)
    if tuple(shape) not in ((3,), (num_drones, 3), full):
        raise ValueError(f"{name} must have shape (3,), ({num_drones}, 3) or {full}, got {tuple(shape)}")


def check_input_shape(name, shape, num_envs, num_drones, width):
    """an input is [E, N, width] exactly"""
    full = (num_envs, num_drones, width)
    if tuple(shape) != full:
        raise ValueError(f"{name} must have shape {full}, got {tuple(shape)}")


class DSLPIDControl:
    """Batched counterpart of gym_pybullet_adrp.control.DSLPIDControl.DSLPIDControl."""

    def __init__(self, drone_model: DroneModel = DroneModel.CF2X, g: float = 9.8, *, num_envs: int = 1,
                 num_drones: int = 1, device: int = 0, precision: str = "fp64"):
        if drone_model not in MIXER_CODE:
            raise ValueError("[ERROR] in DSLPIDControl.__init__(), DSLPIDControl requires DroneModel.CF2X or DroneModel.CF2P")
        if precision not in ("fp32", "fp64"):
            raise ValueError("precision must be 'fp32' or 'fp64'")
        self.lib = _lib.load()
        self.DRONE_MODEL = drone_model
        urdf = URDF_PARAMETERS[drone_model]
        self.GRAVITY = g * urdf["m"]
        self.KF, self.KM = urdf["kf"], urdf["km"]
        p = abi.AdrpDslpidParams()
        self._check_rc(self.lib.adrp_dslpid_default_params(MIXER_CODE[drone_model], ctypes.byref(p)), "adrp_dslpid_default_params")
        p.gravity, p.kf = self.GRAVITY, self.KF
        self._params = p
        self.P_COEFF_FOR, self.I_COEFF_FOR, self.D_COEFF_FOR = (np.array(abi.to_list(getattr(p, f))) for f in _FIELDS[:3])
        self.P_COEFF_TOR, self.I_COEFF_TOR, self.D_COEFF_TOR = (np.array(abi.to_list(getattr(p, f))) for f in _FIELDS[3:])
        self.PWM2RPM_SCALE, self.PWM2RPM_CONST = p.pwm2rpm_scale, p.pwm2rpm_const
        self.MIN_PWM, self.MAX_PWM = p.min_pwm, p.max_pwm
        self.MIXER_MATRIX = np.array(abi.to_list(p.mixer))
        self.num_envs, self.NUM_DRONES = int(num_envs), int(num_drones)
        self.rows = self.num_envs * self.NUM_DRONES
        self.real = torch.float64 if precision == "fp64" else torch.float32
        self.h = None
        c = ctypes.c_void_p()
        rc = self.lib.adrp_dslpid_create(self.rows, int(precision == "fp64"), ctypes.byref(p), int(device), ctypes.byref(c))
        if rc != 0:
            msg = self.lib.adrp_last_error(None).decode()
            raise (ValueError if rc == abi.ERR_INVALID else _lib.AdrpError)(f"adrp_dslpid_create: {msg}")
        self.h = c
        self.device = torch.device("cuda", int(device))
        self._dev_index = self.device.index
        E, N = self.num_envs, self.NUM_DRONES
        self._rpm = torch.zeros((E, N, 4), dtype=self.real, device=self.device)
        self._pos_e = torch.zeros((E, N, 3), dtype=self.real, device=self.device)
        self._yaw_e = torch.zeros((E, N), dtype=self.real, device=self.device)
        self._tbuf = {}      # persistent buffers of broadcast targets
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
            self.lib.adrp_dslpid_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _target(self, name, t):
        """None, or a contiguous [E, N, 3] tensor of the controller's dtype on its device"""
        if t is None:
            return None
        shape = (self.num_envs, self.NUM_DRONES, 3)
        if (isinstance(t, torch.Tensor) and t.dtype == self.real and t.device == self.device and t.shape == shape
                and t.is_contiguous()):
            return t
        t = torch.as_tensor(t, dtype=self.real, device=self.device)
        check_target_shape(name, t.shape, self.num_envs, self.NUM_DRONES)
        buf = self._tbuf.get(name)
        if buf is None:
            buf = self._tbuf[name] = torch.empty(shape, dtype=self.real, device=self.device)
        buf.copy_(t.expand(shape))
        return buf

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

    def _outs(self, out):
        if out is None:
            return self._rpm, self._pos_e, self._yaw_e
        if len(out) != 3:
            raise ValueError("out must be (rpm, pos_e, yaw_e)")
        for old, new in zip((self._rpm, self._pos_e, self._yaw_e), out):
            if new is None:
                continue
            if new.shape != old.shape or new.dtype != old.dtype or new.device != old.device or not new.is_contiguous():
                raise ValueError(f"out: need a contiguous {old.dtype} {tuple(old.shape)} tensor on {old.device}")
        if out[0] is None:
            raise ValueError("out: rpm is required")
        return tuple(out)

    # ---- the reference's surface, batched ----
    def reset(self, mask=None):
        """DSLPIDControl.reset: zero every controller, or those selected by mask ([E] envs or [E, N]
        controllers, non-zero = reset); control_counter restarts as BaseControl.reset does."""
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8)
            if m.shape == (self.num_envs,):
                m = m[:, None].expand(self.num_envs, self.NUM_DRONES)
            if m.shape != (self.num_envs, self.NUM_DRONES):
                raise ValueError(f"mask must have shape ({self.num_envs},) or ({self.num_envs}, {self.NUM_DRONES})")
            m = m.contiguous()
        self._check_rc(self.lib.adrp_dslpid_reset(self.h, _lib._p(m), self._stream()), "adrp_dslpid_reset")
        self.control_counter = 0

    def setPIDCoefficients(self, p_coeff_pos=None, i_coeff_pos=None, d_coeff_pos=None, p_coeff_att=None,
                           i_coeff_att=None, d_coeff_att=None):
        """BaseControl.setPIDCoefficients: replace the given gain triples; later calls use them (a captured
        graph keeps the gains it was captured with)."""
        given = dict(zip(_GAINS, (p_coeff_pos, i_coeff_pos, d_coeff_pos, p_coeff_att, i_coeff_att, d_coeff_att)))
        for key, field, attr in zip(_GAINS, _FIELDS, ("P_COEFF_FOR", "I_COEFF_FOR", "D_COEFF_FOR", "P_COEFF_TOR",
                                                      "I_COEFF_TOR", "D_COEFF_TOR")):
            if given[key] is None:
                continue
            v = np.asarray(given[key], float)
            if v.shape != (3,):
                raise ValueError(f"{key} must have shape (3,)")
            abi.set_vec(getattr(self._params, field), v)
            setattr(self, attr, v.copy())
        self._check_rc(self.lib.adrp_dslpid_set_gains(self.h, ctypes.byref(self._params)), "adrp_dslpid_set_gains")

    def computeControl(self, control_timestep, cur_pos, cur_quat, cur_vel, cur_ang_vel, target_pos, target_rpy=None,
                       target_vel=None, target_rpy_rates=None, out=None):
        """cur_pos / cur_vel [E, N, 3], cur_quat [E, N, 4] (xyzw); cur_ang_vel is unused, as in the reference.
        Returns (rpm [E, N, 4], pos_e [E, N, 3], yaw_e [E, N]) in the controller's dtype."""
        pos, quat, vel = self._input("cur_pos", cur_pos, 3), self._input("cur_quat", cur_quat, 4), self._input("cur_vel", cur_vel, 3)
        if not (pos.dtype == quat.dtype == vel.dtype):
            raise ValueError("cur_pos, cur_quat and cur_vel must share a dtype")
        ip = self._in_precision(pos.dtype)
        rpm, pos_e, yaw_e = self._outs(out)
        t = [self._target(n, v) for n, v in (("target_pos", target_pos), ("target_rpy", target_rpy),
                                             ("target_vel", target_vel), ("target_rpy_rates", target_rpy_rates))]
        self._check_rc(self.lib.adrp_dslpid_compute(self.h, float(control_timestep), _lib._p(pos), _lib._p(quat), _lib._p(vel),
                                                    0, ip, *[_lib._p(x) for x in t], _lib._p(rpm), _lib._p(pos_e),
                                                    _lib._p(yaw_e), self._stream()), "adrp_dslpid_compute")
        self.control_counter += 1
        return rpm, pos_e, yaw_e

    def computeControlFromState(self, control_timestep, state, target_pos, target_rpy=None, target_vel=None,
                                target_rpy_rates=None, out=None):
        """state: a contiguous [E, N, 20] tensor of _getDroneStateVector rows, or a CtrlAviary /
        VelocityAviary / MultiHoverAviary / HoverAviary (the kernel then reads the env's own state columns)."""
        rpm, pos_e, yaw_e = self._outs(out)
        t = [self._target(n, v) for n, v in (("target_pos", target_pos), ("target_rpy", target_rpy),
                                             ("target_vel", target_vel), ("target_rpy_rates", target_rpy_rates))]
        tp = [_lib._p(x) for x in t]
        handle = getattr(state, "h", None)
        if isinstance(handle, _lib.Handle):
            if handle.E * handle.N != self.rows or handle.real != self.real:
                raise ValueError(f"the env has {handle.E} x {handle.N} drones in {handle.real}; the controller "
                                 f"{self.num_envs} x {self.NUM_DRONES} in {self.real}")
            self._check_rc(self.lib.adrp_dslpid_compute_env(self.h, float(control_timestep), handle.h, *tp, _lib._p(rpm),
                                                            _lib._p(pos_e), _lib._p(yaw_e), self._stream()),
                           "adrp_dslpid_compute_env")
        else:
            rows = self._input("state", state, 20)
            ip = self._in_precision(rows.dtype)
            base, sz = rows.data_ptr(), rows.element_size()
            self._check_rc(self.lib.adrp_dslpid_compute(self.h, float(control_timestep), ctypes.c_void_p(base),
                                                        ctypes.c_void_p(base + 3 * sz), ctypes.c_void_p(base + 10 * sz), 20, ip,
                                                        *tp, _lib._p(rpm), _lib._p(pos_e), _lib._p(yaw_e), self._stream()),
                           "adrp_dslpid_compute")
        self.control_counter += 1
        return rpm, pos_e, yaw_e

    # ---- controller state: [9, E * N] = last_rpy 3, integral_pos_e 3, integral_rpy_e 3 ----
    def get_state(self):
        st = torch.empty((9, self.rows), dtype=self.real, device=self.device)
        self._check_rc(self.lib.adrp_dslpid_get_state(self.h, _lib._p(st), self._stream()), "adrp_dslpid_get_state")
        return st

    def set_state(self, st):
        st = torch.as_tensor(st).to(device=self.device, dtype=self.real).contiguous()
        if st.shape != (9, self.rows):
            raise ValueError(f"state must have shape (9, {self.rows}), got {tuple(st.shape)}")
        self._check_rc(self.lib.adrp_dslpid_set_state(self.h, _lib._p(st), self._stream()), "adrp_dslpid_set_state")
