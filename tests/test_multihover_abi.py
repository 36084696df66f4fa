"""MultiHoverAviary C-ABI checks that need no GPU: the task code, its default config, the kernel
naming (lane-group width), the config refusals before any device call, and no CPU fallback."""
import ctypes
import os
import re

import numpy as np
import pytest

from gym_pybullet_adrp_amd.utils import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adrp.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "multihover_golden.npz")


@pytest.fixture(scope="module")
def lib():
    from gym_pybullet_adrp_amd import _lib
    return _lib.load()


def test_header_and_library_agree(lib):
    src = open(HEADER).read()
    assert re.search(r"#define\s+ADRP_TASK_MULTIHOVER\s+2\b", src)
    assert abi.TASK_MULTIHOVER == 2
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    missing = [f for f in sorted(set(re.findall(r"\b(adrp_[a-z_0-9]+)\s*\(", src))) if not hasattr(lib, f)]
    assert not missing, missing
    assert lib.adrp_abi_version() == abi.ABI_VERSION


def test_default_config(lib):
    from gym_pybullet_adrp_amd import _lib
    cfg = _lib.default_config(abi.TASK_MULTIHOVER)
    hov = _lib.default_config(abi.TASK_HOVER)
    assert cfg.struct_size == ctypes.sizeof(abi.AdrpConfig) == hov.struct_size   # the config struct is unchanged
    assert cfg.task == abi.TASK_MULTIHOVER and cfg.num_drones == 2
    fx = np.load(GOLDEN)
    np.testing.assert_array_equal(np.array(abi.to_list(cfg.init_xyz))[:2], fx["rpm2_init_xyzs"])
    # everything else is the hover default
    cfg.task, cfg.num_drones = hov.task, hov.num_drones
    abi.set_vec(cfg.init_xyz[1], [0.0, 0.0, 0.0])
    assert bytes(cfg) == bytes(hov)


@pytest.mark.parametrize("n,g", [(1, 1), (2, 2), (3, 4), (5, 8), (8, 8)])
def test_kernel_name(lib, n, g):
    from gym_pybullet_adrp_amd import _lib
    cfg = _lib.default_config(abi.TASK_MULTIHOVER)
    cfg.num_drones = n
    assert _lib.kernel_name(cfg) == f"multihover_step<f32,PYB,A4,G{g}>"
    cfg.precision, cfg.physics, cfg.act_type = 1, abi.PHYS_PYB_GND_DRAG_DW, abi.ACT_ONE_D_RPM
    assert _lib.kernel_name(cfg) == f"multihover_step<f64,PYB_GND_DRAG_DW,A1,G{g}>"
    cfg.physics = abi.PHYS_DYN
    assert _lib.kernel_name(cfg) == f"multihover_step<f64,DYN,A1,G{g}>"


@pytest.mark.parametrize("field,value,msg", [
    ("num_drones", 0, b"MultiHoverAviary num_drones must be 1..8"),
    ("num_drones", 9, b"MultiHoverAviary num_drones must be 1..8"),
    ("act_type", abi.ACT_PID, b"PID"), ("act_type", abi.ACT_VEL, b"VEL"), ("act_type", abi.ACT_ONE_D_PID, b"ONE_D_PID"),
    ("act_type", abi.ACT_FULLSTATE, b"RPM or ONE_D_RPM"), ("num_envs", 0, b"num_envs"), ("physics", 9, b"physics")])
def test_refused_before_device(lib, field, value, msg):
    from gym_pybullet_adrp_amd import _lib
    cfg = _lib.default_config(abi.TASK_MULTIHOVER)
    setattr(cfg, field, value)
    h = ctypes.c_void_p()
    assert lib.adrp_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == abi.ERR_INVALID
    assert msg in lib.adrp_last_error(None), lib.adrp_last_error(None)
    assert not h.value


def test_hover_task_still_has_one_drone(lib):
    from gym_pybullet_adrp_amd import _lib
    cfg = _lib.default_config(abi.TASK_HOVER)
    cfg.num_drones = 2
    h = ctypes.c_void_p()
    assert lib.adrp_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == abi.ERR_INVALID
    assert b"exactly one drone" in lib.adrp_last_error(None)


def test_no_cpu_fallback(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from gym_pybullet_adrp_amd import _lib
    from gym_pybullet_adrp_amd.envs import MultiHoverAviary
    cfg = _lib.default_config(abi.TASK_MULTIHOVER)
    h = ctypes.c_void_p()
    assert lib.adrp_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == abi.ERR_DEVICE
    with pytest.raises(_lib.AdrpError):
        MultiHoverAviary(num_envs=4)


def test_not_in_the_registry():
    """the env is exported from `envs`; the registry stays the reference's two race-relevant ids"""
    import gym_pybullet_adrp_amd as pkg
    from gym_pybullet_adrp_amd import envs, vec_env
    assert hasattr(envs, "MultiHoverAviary") and hasattr(vec_env, "MultiHoverAviaryVec")
    assert not any("multihover" in k.lower() for k in pkg.ENV_IDS)
