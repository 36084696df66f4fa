"""C-ABI surface of the on-device PPO update (include/adrp.h adrp_ppo_*, csrc/ppo.hip), the part
that needs no GPU: the header / library / ctypes mirror agree, every refusal that can be reached
without a device handle names its cause and leaves ``out`` NULL, ``PPOLearner`` refuses to run
without a GPU, and the float64 loss the GPU tests measure against (tests/ppo_reference.py)
reproduces a two-row case computed by hand.

(The refusal of a policy without a critic needs a policy handle, which only a GPU machine can
create: tests/test_ppo_update_gpu.py holds it.)"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from gym_pybullet_adrp_amd import _lib
from gym_pybullet_adrp_amd.utils import abi
from tests import ppo_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PPO_FUNCTIONS = {"adrp_ppo_default_cfg", "adrp_ppo_create", "adrp_ppo_update", "adrp_ppo_param_count", "adrp_ppo_params",
                 "adrp_ppo_set_params", "adrp_ppo_gradients", "adrp_ppo_destroy"}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_declares_and_library_exports_the_ppo_functions(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adrp.h")).read(), flags=re.S)
    declared = {f for f in re.findall(r"\b(adrp_[a-z_]+)\s*\(", src) if f.startswith("adrp_ppo_")}
    assert declared == PPO_FUNCTIONS
    assert not [f for f in declared if not hasattr(lib, f)]
    assert "#define ADRP_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "adrp.h")).read()


def test_cfg_mirror_and_defaults(lib):
    cfg = abi.AdrpPpoCfg()
    assert lib.adrp_ppo_default_cfg(ctypes.byref(cfg)) == abi.OK
    assert cfg.struct_size == ctypes.sizeof(abi.AdrpPpoCfg)
    got = (cfg.learning_rate, cfg.clip_range, cfg.clip_range_vf, cfg.ent_coef, cfg.vf_coef, cfg.max_grad_norm,
           cfg.normalize_advantage)
    assert got == (3e-4, 0.2, -1.0, 0.0, 0.5, 0.5, 1)          # SB3 PPO's defaults; clip_range_vf < 0 is None


def _create(lib, policy, **change):
    cfg = abi.AdrpPpoCfg()
    lib.adrp_ppo_default_cfg(ctypes.byref(cfg))
    for k, v in change.items():
        setattr(cfg, k, v)
    out = ctypes.c_void_p(0xdead)
    rc = lib.adrp_ppo_create(policy, ctypes.byref(cfg), ctypes.byref(out))
    return rc, out.value, lib.adrp_last_error(None).decode()


@pytest.mark.parametrize("change, word", [
    (dict(), "policy is NULL"),
    (dict(struct_size=8), "struct_size"),
    (dict(learning_rate=0.0), "learning_rate"),
    (dict(learning_rate=-1e-3), "learning_rate"),
    (dict(learning_rate=float("nan")), "learning_rate"),
    (dict(clip_range=-0.1), "clip_range"),
])
def test_create_refusals(lib, change, word):
    """checked before any device call: they answer on a machine without a GPU.  The cfg is checked
    before the policy, so a NULL policy reaches each of them."""
    rc, out, msg = _create(lib, None, **change)
    assert rc == abi.ERR_INVALID
    assert out is None                                         # *out = NULL
    assert word in msg and msg.startswith("adrp_ppo_create")


def test_update_refuses_an_empty_minibatch(lib):
    """n < 1 is refused before the handle is looked at"""
    for n in (0, -3):
        assert lib.adrp_ppo_update(None, None, 0, None, None, None, None, None, None, n, None, None) == abi.ERR_INVALID
        assert "n must be at least 1" in lib.adrp_last_error(None).decode()
    assert lib.adrp_ppo_update(None, None, 0, None, None, None, None, None, None, 4, None, None) == abi.ERR_INVALID
    assert "NULL" in lib.adrp_last_error(None).decode()


def test_learner_needs_a_gpu(monkeypatch):
    from gym_pybullet_adrp_amd.ppo import PPOLearner
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.AdrpError, match="no HIP device"):
        PPOLearner(object())


def test_reference_loss_two_rows_by_hand():
    """The yardstick pinned on a case small enough for a pencil: a 1 -> 16 -> 16 -> 1 ReLU policy whose
    hidden layers pass obs[0] = 1 through one unit (mean = w3 = 0.5 on both rows, value 2), sigma = 1,
    clip 0.2, no advantage normalisation.  Row 0: action 1.5, old_log_prob = log_prob - log 1.5, so ratio
    1.5 > 1.2 with advantage +2: the clipped branch is the smaller one, its gradient zero.  Row 1:
    action 0, old_log_prob = log_prob - log 1.1, ratio 1.1 inside the range with advantage -1."""
    w = {k: np.zeros(s, np.float32) for k, s in zip(R.KEYS, [(16, 1), (16,), (16, 16), (16,), (1, 16), (1,)] * 2 + [(1,)])}
    for pre, head, out in (("policy_net", "action_net", 0.5), ("value_net", "value_net", 2.0)):
        w[f"mlp_extractor.{pre}.0.weight"][0, 0] = 1.0
        w[f"mlp_extractor.{pre}.2.weight"][0, 0] = 1.0
        w[f"{head}.weight"][0, 0] = out
    c = math.log(math.sqrt(2 * math.pi))
    lp = np.array([-0.5 * 1.0 ** 2 - c, -0.5 * 0.5 ** 2 - c])            # actions 1.5, 0 around mean 0.5
    old_lp = lp - np.log([1.5, 1.1])
    batch = (np.ones((2, 1)), np.array([[1.5], [0.0]]), np.array([2.0, 2.0]), old_lp, np.array([2.0, -1.0]),
             np.array([3.0, 1.5]))
    cfg = R.config(normalize_advantage=False, ent_coef=0.0, vf_coef=0.5)
    g, stats, rows = R.gradients(w, batch, cfg, True, torch.float64)
    assert rows["zero_grad"].tolist() == [True, False] and rows["unclipped"].tolist() == [False, True]
    assert np.allclose(rows["ratio"].numpy(), [1.5, 1.1], rtol=1e-12)
    # policy_loss = -mean(min(2 * 1.5, 2 * 1.2), min(-1.1, -1.1)) = -(2.4 - 1.1) / 2
    assert stats["policy_loss"] == pytest.approx(-0.65, rel=1e-12)
    assert stats["value_loss"] == pytest.approx(((3.0 - 2.0) ** 2 + (1.5 - 2.0) ** 2) / 2, rel=1e-12)
    assert stats["clip_fraction"] == 0.5
    assert stats["entropy_loss"] == pytest.approx(-(0.5 + 0.5 * math.log(2 * math.pi)), rel=1e-12)
    assert stats["approx_kl"] == pytest.approx(((0.5 - math.log(1.5)) + (0.1 - math.log(1.1))) / 2, rel=1e-12)
    # only row 1 reaches the actor: d loss / d log_prob = -adv ratio / 2 = 0.55, d log_prob / d mean = a - mean = -0.5
    assert float(g["action_net.bias"][0]) == pytest.approx(0.55 * -0.5, rel=1e-12)
    assert float(g["action_net.weight"][0, 0]) == pytest.approx(0.55 * -0.5 * 1.0, rel=1e-12)   # hidden unit = 1
    # d log_prob / d log_std = (a - mean)^2 / sigma^2 - 1 = -0.75 on row 1
    assert float(g["log_std"][0]) == pytest.approx(0.55 * -0.75, rel=1e-12)
    # value: vf_coef * 2 (v - ret) / 2 summed over both rows = 0.5 * ((2 - 3) + (2 - 1.5))
    assert float(g["value_net.bias"][0]) == pytest.approx(0.5 * (-1.0 + 0.5), rel=1e-12)
    # clip_range_vf: values_pred = old_values + clamp(v - old_values): with old value 1 and c_vf 0.2 the value
    # is clipped to 1.2 and its gradient vanishes
    cfg2 = R.config(normalize_advantage=False, clip_range_vf=0.2)
    batch2 = batch[:2] + (np.array([1.0, 2.0]),) + batch[3:]
    g2, stats2, _ = R.gradients(w, batch2, cfg2, True, torch.float64)
    assert stats2["value_loss"] == pytest.approx(((3.0 - 1.2) ** 2 + (1.5 - 2.0) ** 2) / 2, rel=1e-12)
    assert float(g2["value_net.bias"][0]) == pytest.approx(0.5 * 0.5, rel=1e-12)


def test_reference_clip_adam_matches_torch():
    """the written-out clip + Adam step of the yardstick is torch's own (float64), above and below the norm bound"""
    w = R.make_weights(5, 16, 16, 2, 0)
    rng = np.random.default_rng(1)
    for scale in (10.0, 1e-3):
        p = R.to_params(w, torch.float64)
        grads = {k: torch.tensor(rng.normal(size=w[k].shape) * scale) for k in R.KEYS}
        opt = torch.optim.Adam([p[k] for k in R.KEYS], lr=3e-4, eps=1e-5)
        for k in R.KEYS:
            p[k].grad = grads[k].clone()
        torch.nn.utils.clip_grad_norm_([p[k] for k in R.KEYS], 0.5)
        opt.step()
        zero = {k: torch.zeros_like(grads[k]) for k in R.KEYS}
        po, _, _, t, norm = R.clip_adam({k: torch.tensor(w[k]).double() for k in R.KEYS}, grads, zero, zero, 0, R.config())
        assert t == 1 and (norm > 0.5) == (scale > 1)
        for k in R.KEYS:
            assert torch.allclose(po[k], p[k].detach(), rtol=1e-12, atol=1e-15)
