"""Wide on-device policy path (csrc/policy_kernel.h policy_wide_kernel / policy_sample_wide_kernel:
in_dim <= 576, act_dim <= 32), CPU part: the host's MFMA fragment blob decoded back through the
documented lane map, the argument checks of adrp_policy_create2 and the zip loader at a joint
MultiHoverAviary shape.  The kernels themselves: tests/test_policy_wide_gpu.py."""
import ctypes
import io
import json
import zipfile

import numpy as np
import pytest
import torch

from gym_pybullet_adrp_amd import _lib
from gym_pybullet_adrp_amd.policy import ACTOR_KEYS, CRITIC_KEYS, load_sb3_zip, policy_fragments
from gym_pybullet_adrp_amd.utils import abi
from oracle import policy as OP


def random_net(rng, in_dim, h1, h2, out):
    """{ACTOR_KEYS + CRITIC_KEYS: float32} of a random two-hidden-layer actor / critic:
    W ~ N(0, sqrt(2 / fan_in)), the action / value head scaled by 0.3, biases ~ N(0, 0.1),
    log_std ~ U(-1, 0): with obs ~ U(-2, 2) the pre-activations stay O(1), tanh does not saturate and a
    dropped or misplaced input column shows as an error of order 0.1"""
    def lin(o, i, scale=1.0):
        return ((rng.standard_normal((o, i)) * np.sqrt(2.0 / i) * scale).astype(np.float32),
                (rng.standard_normal(o) * 0.1).astype(np.float32))
    a = lin(h1, in_dim) + lin(h2, h1) + lin(out, h2, 0.3)
    c = lin(h1, in_dim) + lin(h2, h1) + lin(1, h2, 0.3) + (rng.uniform(-1, 0, out).astype(np.float32),)
    wd = dict(zip(ACTOR_KEYS, a))
    wd.update(zip(CRITIC_KEYS, c))
    return wd


def actor(wd):
    return [wd[k] for k in ACTOR_KEYS]


def critic(wd):
    return [wd[k] for k in CRITIC_KEYS]


def random_obs(rng, shape):
    return rng.uniform(-2, 2, shape).astype(np.float32)


def decode(blob, L, h1, h2):
    """the blob back into (W1 [h1, 4 s1], b1, W2, b2, W3 [16 t3, h2], b3 [16 t3]) through the lane map of
    include/adrp.h adrp_policy_fragments; every blob float is visited exactly once (checked)"""
    T1, T2, S1, T3 = h1 // 16, h2 // 16, L["s1"], L["t3"]
    seen = np.zeros(blob.size, bool)
    lane = np.arange(64)
    lo, hi = lane & 15, lane >> 4

    def take(off):
        assert not seen[off:off + 64].any()
        seen[off:off + 64] = True
        return blob[off:off + 64]
    W1 = np.zeros((h1, 4 * S1), np.float32)
    for t in range(T1):
        for s in range(S1):
            W1[16 * t + lo, 4 * s + hi] = take(L["f1"] + (t * S1 + s) * 64)
    W2 = np.zeros((h2, h1), np.float32)
    for u in range(T2):
        for t in range(T1):
            for i in range(4):
                W2[16 * u + lo, 16 * t + 4 * hi + i] = take(L["f2"] + ((u * T1 + t) * 4 + i) * 64)
    W3 = np.zeros((16 * T3, h2), np.float32)
    for u3 in range(T3):
        for u in range(T2):
            for i in range(4):
                W3[16 * u3 + lo, 16 * u + 4 * hi + i] = take(L["f3"] + ((u3 * T2 + u) * 4 + i) * 64)
    for off, n in ((L["b1"], h1), (L["b2"], h2), (L["b3"], 16 * T3)):
        assert not seen[off:off + n].any()
        seen[off:off + n] = True
    assert L["f1"] == 0 and L["total"] == blob.size and not seen[L["b3"] + 16 * T3:].any()
    assert seen[:L["b3"] + 16 * T3].all()                 # no gap between the sections
    assert not blob[L["b3"] + 16 * T3:].any()             # the round-up to 4 floats
    return W1, blob[L["b1"]:L["b1"] + h1], W2, blob[L["b2"]:L["b2"] + h2], W3, blob[L["b3"]:L["b3"] + 16 * T3]


FRAGMENT_SHAPES = [(72, 64, 64, 4, 1), (81, 16, 128, 3, 1), (144, 64, 64, 8, 1), (216, 128, 32, 12, 1),
                   (576, 64, 64, 32, 1), (49, 64, 64, 4, 0), (49, 64, 64, 4, 1)]


@pytest.mark.parametrize("in_dim,h1,h2,out,wide", FRAGMENT_SHAPES)
def test_fragments_decode_to_the_weights(in_dim, h1, h2, out, wide):
    rng = np.random.default_rng(in_dim + out)
    wd = random_net(rng, in_dim, h1, h2, out)
    w = actor(wd)
    blob, L = policy_fragments(wd, wide=bool(wide))
    s1 = -(-in_dim // 4)
    chunked = -(-s1 // 16) * 16
    assert L["in_dim"] == in_dim and L["n_out"] == out and L["t3"] == -(-out // 16)
    assert L["s1"] == (chunked if (wide or in_dim > 64 or out > 4) else 16)
    assert L["wide"] == int(bool(wide) or in_dim > 64 or out > 4)
    W1, b1, W2, b2, W3, b3 = decode(blob, L, h1, h2)
    np.testing.assert_array_equal(W1[:, :in_dim], w[0])
    assert not W1[:, in_dim:].any()                        # zero weights on the padded k-steps
    np.testing.assert_array_equal(b1, w[1])
    np.testing.assert_array_equal(W2, w[2])
    np.testing.assert_array_equal(b2, w[3])
    np.testing.assert_array_equal(W3[:out], w[4])
    assert not W3[out:].any()                              # zero rows beyond act_dim
    np.testing.assert_array_equal(b3[:out], w[5])
    assert not b3[out:].any()
    # the decoded matrices are the network: a float64 forward over the padded width equals the oracle's
    # (the zero padding only regroups BLAS's float64 sums: 1e-13 on O(1) outputs)
    x = random_obs(rng, (33, in_dim))
    xp = np.zeros((33, W1.shape[1]), np.float32)
    xp[:, :in_dim] = x
    got = OP.actor_mean((W1, b1, W2, b2, W3, b3), xp, False)
    np.testing.assert_allclose(got[:, :out], OP.actor_mean(w, x, False), rtol=0, atol=1e-13)
    assert not got[:, out:].any()


def test_narrow_and_wide_blob_of_a_narrow_policy_are_the_same():
    """49 -> 4: one chunk and one output tile, so ADRP_POLICY_WIDE=1 uploads the bytes the narrow kernels read"""
    wd = random_net(np.random.default_rng(1), 49, 64, 64, 4)
    (b0, L0), (b1, L1) = policy_fragments(wd, wide=False), policy_fragments(wd, wide=True)
    np.testing.assert_array_equal(b0, b1)
    assert {k: v for k, v in L0.items() if k != "wide"} == {k: v for k, v in L1.items() if k != "wide"}


def test_fragments_capacity_and_refusals():
    lib = _lib.load()
    wd = random_net(np.random.default_rng(2), 72, 16, 16, 4)
    ptr = [a.ctypes.data_as(ctypes.c_void_p) for a in actor(wd)]
    n = lib.adrp_policy_fragments(72, 16, 16, 4, *ptr, 0, None, 0, None)
    assert n > 0
    small = np.full(n, 7.0, np.float32)
    assert lib.adrp_policy_fragments(72, 16, 16, 4, *ptr, 0, small.ctypes.data_as(ctypes.c_void_p), n - 1, None) == n
    assert (small == 7.0).all()                            # too small a buffer is left alone
    assert lib.adrp_policy_fragments(577, 16, 16, 4, *ptr, 0, None, 0, None) == abi.ERR_INVALID
    assert lib.adrp_policy_fragments(72, 16, 16, 33, *ptr, 0, None, 0, None) == abi.ERR_INVALID
    assert lib.adrp_policy_fragments(72, 48, 16, 4, *ptr, 0, None, 0, None) == abi.ERR_INVALID


def _create(in_dim, act_dim, h=16):
    lib = _lib.load()
    z = [np.zeros(n, np.float32) for n in (h * in_dim if in_dim > 0 else 1, h, h * h, h, h * max(act_dim, 1), max(act_dim, 1))]
    handle = ctypes.c_void_p()
    rc = lib.adrp_policy_create2(0, in_dim, h, h, act_dim, abi.POLICY_TANH, *[a.ctypes.data_as(ctypes.c_void_p) for a in z],
                                 ctypes.byref(handle))
    msg = lib.adrp_last_error(None).decode()
    if rc == 0:
        lib.adrp_policy_destroy(handle)
    return rc, msg


@pytest.mark.parametrize("in_dim,act_dim", [(72, 4), (576, 32), (65, 5)])
def test_create_accepts_wide_shapes(in_dim, act_dim):
    """outside the narrow box is no longer an argument error: the create gets as far as the device"""
    rc, msg = _create(in_dim, act_dim)
    assert rc in (0, abi.ERR_DEVICE), msg


@pytest.mark.parametrize("in_dim,act_dim,msg", [(577, 4, "policy in_dim must be 1..576"),
                                                (64, 33, "policy act_dim must be 1..32"),
                                                (0, 4, "policy in_dim must be 1..576")])
def test_create_refuses_beyond_the_wide_bounds(in_dim, act_dim, msg):
    rc, got = _create(in_dim, act_dim)
    assert rc == abi.ERR_INVALID and msg in got


def test_zip_round_trip_joint_shape(tmp_path):
    """an SB3-layout zip of a joint two-drone MultiHoverAviary(RPM) policy: 144 -> 64 -> 64 -> 8, a critic
    and log_std[8]"""
    wd = random_net(np.random.default_rng(3), 144, 64, 64, 8)
    buf = io.BytesIO()
    torch.save({k: torch.from_numpy(v) for k, v in wd.items()}, buf)
    path = str(tmp_path / "joint.zip")
    with zipfile.ZipFile(path, "w") as zf:
        zf.writestr("data", json.dumps({"verbose": 0, "policy_kwargs": {}}))
        zf.writestr("policy.pth", buf.getvalue())
        zf.writestr("_stable_baselines3_version", "2.3.2")
    w, act = load_sb3_zip(path, critic=True)
    assert act == "tanh"
    assert w[ACTOR_KEYS[0]].shape == (64, 144) and w[ACTOR_KEYS[4]].shape == (8, 64)
    assert w[CRITIC_KEYS[0]].shape == (64, 144) and w[CRITIC_KEYS[4]].shape == (1, 64) and w["log_std"].shape == (8,)
    for k in ACTOR_KEYS + CRITIC_KEYS:
        np.testing.assert_array_equal(w[k], wd[k])
