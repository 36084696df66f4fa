"""The target_kl latch and the rate schedules of the on-device PPO update (include/adrp_train.h adrp_ppo_*,
csrc/ppo.hip, gym_pybullet_adrp_amd/ppo.py), the part that needs no GPU: the new entry points are declared and
exported and the ABI version stays, every refusal answers without a device and names its function,
``linear_schedule`` is SB3's ``get_linear_fn``, and the yardstick of the GPU tests (tests/ppo_train_reference.py)
meets the conditions its cases are chosen by, on the reference alone."""
import os
import re

import pytest
import torch

from gym_pybullet_adrp_amd import _lib, ppo
from gym_pybullet_adrp_amd.utils import abi
from tests import ppo_reference as R
from tests import ppo_train_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = {"adrp_ppo_set_target_kl", "adrp_ppo_set_rates", "adrp_ppo_train_begin", "adrp_ppo_stop_state"}
PTR = 0x1000        # never dereferenced: every call below is refused before the first device call


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_declares_and_library_exports_the_new_functions(lib):
    text = open(os.path.join(ROOT, "include", "adrp_train.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = {f for f in re.findall(r"\b(adrp_[a-z_]+)\s*\(", src) if f.startswith("adrp_ppo_")}
    assert declared == NEW_FUNCTIONS
    assert not [f for f in declared if not hasattr(lib, f)]
    main = open(os.path.join(ROOT, "include", "adrp.h")).read()
    assert '#include "adrp_train.h"' in main and "#define ADRP_ABI_VERSION 2" in main
    assert lib.adrp_abi_version() == 2 == abi.ABI_VERSION


@pytest.mark.parametrize("fn, call, word", [
    ("adrp_ppo_set_target_kl", lambda lib: lib.adrp_ppo_set_target_kl(None, 0.01), "ppo is NULL"),
    ("adrp_ppo_set_target_kl", lambda lib: lib.adrp_ppo_set_target_kl(None, -1.0), "ppo is NULL"),
    ("adrp_ppo_set_target_kl", lambda lib: lib.adrp_ppo_set_target_kl(None, float("nan")), "target_kl is NaN"),
    ("adrp_ppo_set_rates", lambda lib: lib.adrp_ppo_set_rates(None, 3e-4, 0.2, -1.0), "ppo is NULL"),
    ("adrp_ppo_set_rates", lambda lib: lib.adrp_ppo_set_rates(None, 0.0, 0.2, -1.0), "learning_rate"),
    ("adrp_ppo_set_rates", lambda lib: lib.adrp_ppo_set_rates(None, -1e-3, 0.2, -1.0), "learning_rate"),
    ("adrp_ppo_set_rates", lambda lib: lib.adrp_ppo_set_rates(None, float("nan"), 0.2, -1.0), "learning_rate"),
    ("adrp_ppo_set_rates", lambda lib: lib.adrp_ppo_set_rates(None, 3e-4, -0.1, -1.0), "clip_range"),
    ("adrp_ppo_set_rates", lambda lib: lib.adrp_ppo_set_rates(None, 3e-4, float("nan"), -1.0), "clip_range"),
    ("adrp_ppo_set_rates", lambda lib: lib.adrp_ppo_set_rates(None, 3e-4, 0.2, float("nan")), "clip_range_vf"),
    ("adrp_ppo_stop_state", lambda lib: lib.adrp_ppo_stop_state(None, None, None), "out_dev2 is NULL"),
    ("adrp_ppo_train_begin", lambda lib: lib.adrp_ppo_train_begin(None, None), "ppo is NULL"),
    ("adrp_ppo_stop_state", lambda lib: lib.adrp_ppo_stop_state(None, PTR, None), "ppo is NULL"),
])
def test_refusals(lib, fn, call, word):
    """the values are checked before the handle (as adrp_ppo_create checks its cfg before its policy), so a NULL
    handle reaches each of them on a machine without a GPU"""
    assert call(lib) == abi.ERR_INVALID
    msg = lib.adrp_last_error(None).decode()
    assert msg.startswith(fn + ":") and word in msg, msg


def test_learner_side_refusals():
    """what ``PPOLearner``'s setters refuse themselves, before the library is called"""
    self = ppo.PPOLearner.__new__(ppo.PPOLearner)
    for bad in (float("nan"), -0.01):
        with pytest.raises(ValueError, match="target_kl"):
            ppo.PPOLearner.set_target_kl(self, bad)
    with pytest.raises(ValueError, match="clip_range_vf"):
        ppo.PPOLearner.set_rates(self, 3e-4, 0.2, -0.1)
    # the stop is switched on by the setter alone: train()'s keyword stays refused, before the collector is looked at
    # (tests/test_ppo_update_gpu.py pins that, and the constructor's, on a device)
    with pytest.raises(ValueError, match="set_target_kl"):
        ppo.PPOLearner.train(self, None, target_kl=0.01)


@pytest.mark.parametrize("end_fraction", [1.0, 0.5])
@pytest.mark.parametrize("progress", [1.0, 0.75, 0.5, 0.1, 0.0])
def test_linear_schedule_is_get_linear_fn(progress, end_fraction):
    start, end = 3e-4, 1e-5
    f = ppo.linear_schedule(start, end, end_fraction)
    want = end if 1 - progress > end_fraction else start + (1 - progress) * (end - start) / end_fraction
    assert f(progress) == want
    assert ppo.linear_schedule(start)(1.0) == start and ppo.linear_schedule(start)(0.0) == 0.0
    assert ppo.linear_schedule(0.2, 0.05, 0.5)(0.25) == 0.05        # past the end fraction: held


@pytest.mark.parametrize("i", range(len(T.CASES)), ids=lambda i: "-".join(map(str, T.CASES[i].shape)))
def test_yardstick_conditions(i):
    """asserted on the reference alone: the trip index is inside the loop, the threshold is far from both of its
    neighbours by the reference's own float32-vs-float64 deviation, and the stop does what SB3's does"""
    c = T.case(i)
    assert len(c.kl64) == len(c.kl32) == c.n
    assert 1 <= c.k < c.n - 1
    assert c.below < c.thr < c.at
    print(f"case {i}: KL64 {['%.3e' % x for x in c.kl64]} k* {c.k} 1.5 target_kl {c.thr:.4e} dev {c.dev:.2e}")
    assert min(c.thr - c.below, c.at - c.thr) >= 100 * c.dev
    for dtype, kls in ((torch.float64, c.kl64), (torch.float32, c.kl32)):
        p, got, trip = T.train_loop_kl(c.w, c.buf, c.perms, c.c.batch, c.cfg, c.relu, dtype, target_kl=c.target_kl)
        assert trip == c.k and got == kls[:c.k + 1]
        # the parameters are those of the loop over the first k* minibatches alone: the tripping one took no step
        full, part = divmod(c.k, c.nmb)
        head = [c.perms[e] for e in range(full)] + ([c.perms[full][:part * c.c.batch]] if part else [])
        p_cut = R.train_loop(c.w, c.buf, head, c.c.batch, c.cfg, c.relu, dtype)
        for key in R.KEYS:
            assert torch.equal(p[key], p_cut[key])
    # a NaN statistic does not trip (the comparison is false), a huge target never does
    assert not float("nan") > 1.5 * c.target_kl
    _, _, never = T.train_loop_kl(c.w, c.buf, c.perms, c.c.batch, c.cfg, c.relu, torch.float32, target_kl=1e9)
    assert never is None


def test_cases_cover_first_of_an_epoch_and_mid_epoch():
    at = [T.case(i).k % T.case(i).nmb for i in range(len(T.CASES))]
    assert 0 in at and any(a != 0 for a in at)
    assert {T.CASES[i].activation for i in range(len(T.CASES))} == {"tanh", "relu"}


def test_reference_without_a_target_is_train_loop():
    c = T.case(0)
    p, _, trip = T.train_loop_kl(c.w, c.buf, c.perms, c.c.batch, c.cfg, c.relu, torch.float64)
    q = R.train_loop(c.w, c.buf, c.perms, c.c.batch, c.cfg, c.relu, torch.float64)
    assert trip is None
    for key in R.KEYS:
        assert torch.equal(p[key], q[key])
