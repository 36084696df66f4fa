"""C-ABI surface of the on-device episode statistics (include/adrp.h adrp_episode_*, csrc/episode.hip)
and the host-side logic of gym_pybullet_adrp_amd/evaluation.py, the part that needs no GPU: the header /
library / ctypes mirror agree, every refusal is reached without a device and names its cause,
``EpisodeStats`` and ``evaluate_policy`` refuse to run without a GPU, SB3's episode_count_targets, the
numpy yardstick (tests/episode_reference.py) on a case computed by hand, and the ``Evaluator``'s
schedule / best / threshold logic with the evaluation itself stubbed."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from gym_pybullet_adrp_amd import _lib, evaluation
from gym_pybullet_adrp_amd.utils import abi
from tests import episode_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPISODE_FUNCTIONS = {"adrp_episode_step", "adrp_episode_summary"}
BUFFERS = ("run_return", "run_length", "count", "meta", "log_return", "log_length", "log_env")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_declares_and_library_exports_the_episode_functions(lib):
    text = open(os.path.join(ROOT, "include", "adrp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = {f for f in re.findall(r"\b(adrp_[a-z_]+)\s*\(", src) if f.startswith("adrp_episode_")}
    assert declared == EPISODE_FUNCTIONS
    assert not [f for f in declared if not hasattr(lib, f)]
    assert "#define ADRP_ABI_VERSION 2" in text           # purely additive: the ABI version stays


def _io(**change):
    """a well-formed adrp_episode_io (the pointers are never dereferenced by a refusal)"""
    io = abi.AdrpEpisodeIO()
    io.struct_size = ctypes.sizeof(abi.AdrpEpisodeIO)
    io.num_envs, io.capacity, io.ring = 4, 10, 1
    io.quota = None
    for k in BUFFERS:
        setattr(io, k, 0x1000)
    for k, v in change.items():
        setattr(io, k, v)
    return io


def test_struct_mirror():
    """the header's struct on LP64: four 32-bit fields, eight pointers"""
    assert ctypes.sizeof(abi.AdrpEpisodeIO) == 4 * 4 + 8 * 8
    assert [f[0] for f in abi.AdrpEpisodeIO._fields_] == ["struct_size", "num_envs", "capacity", "ring", "quota"] + list(BUFFERS)
    text = open(os.path.join(ROOT, "include", "adrp.h")).read()
    body = re.search(r"typedef struct adrp_episode_io \{(.*?)\} adrp_episode_io;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*;", body)
    assert names == [f[0] for f in abi.AdrpEpisodeIO._fields_]


REFUSALS = [(dict(struct_size=8), "struct_size"), (dict(struct_size=ctypes.sizeof(abi.AdrpEpisodeIO) + 8), "struct_size"),
            (dict(num_envs=0), "num_envs"), (dict(num_envs=-3), "num_envs"),
            (dict(capacity=0), "capacity"), (dict(ring=2), "ring"), (dict(ring=-1), "ring")] \
    + [({k: None}, "NULL buffer") for k in BUFFERS]


@pytest.mark.parametrize("change, word", REFUSALS)
def test_io_refusals(lib, change, word):
    """checked before any device call: they answer on a machine without a GPU.  A wrong struct_size is
    what a caller built against another header shows, so it is checked first."""
    io = _io(**change)
    for fn, call in (("adrp_episode_step", lambda: lib.adrp_episode_step(ctypes.byref(io), 0x1000, 0x1000, 0x1000, None)),
                     ("adrp_episode_summary", lambda: lib.adrp_episode_summary(ctypes.byref(io), 0x1000, None))):
        assert call() == abi.ERR_INVALID
        msg = lib.adrp_last_error(None).decode()
        assert msg.startswith(fn) and word in msg


def test_null_refusals(lib):
    assert lib.adrp_episode_step(None, 0x1000, 0x1000, 0x1000, None) == abi.ERR_INVALID
    assert lib.adrp_last_error(None).decode() == "adrp_episode_step: io is NULL"
    assert lib.adrp_episode_summary(None, 0x1000, None) == abi.ERR_INVALID
    assert lib.adrp_last_error(None).decode() == "adrp_episode_summary: io is NULL"
    io = _io()                       # a NULL quota is fine: the refusal below is about the step's inputs
    for args in ((None, 0x1000, 0x1000), (0x1000, None, 0x1000), (0x1000, 0x1000, None)):
        assert lib.adrp_episode_step(ctypes.byref(io), *args, None) == abi.ERR_INVALID
        msg = lib.adrp_last_error(None).decode()
        assert msg.startswith("adrp_episode_step") and "NULL" in msg and "rew / term / trunc" in msg
    assert lib.adrp_episode_summary(ctypes.byref(io), None, None) == abi.ERR_INVALID
    msg = lib.adrp_last_error(None).decode()
    assert msg.startswith("adrp_episode_summary") and "out8" in msg


def _stub_env():
    cfg = types.SimpleNamespace(autoreset=1, task=abi.TASK_HOVER, episode_len_sec=8.0)
    return types.SimpleNamespace(cfg=cfg, NUM_DRONES=1, num_envs=2, CTRL_FREQ=30, device=torch.device("cuda", 0))


def test_episode_stats_and_evaluate_policy_need_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)      # (as tests/test_ppo_abi.py: no skip with a GPU)
    with pytest.raises(_lib.AdrpError, match="no HIP device"):
        evaluation.EpisodeStats(4, 0)
    with pytest.raises(_lib.AdrpError, match="no HIP device"):
        evaluation.evaluate_policy(object(), _stub_env(), n_eval_episodes=2)


@pytest.mark.parametrize("n, E, want", [(7, 5, [1, 1, 1, 2, 2]), (3, 5, [0, 0, 1, 1, 1]), (10, 1, [10]),
                                        (1300, 1025, [1] * 750 + [2] * 275)])
def test_quota_vectors(n, E, want):
    q = evaluation.episode_count_targets(n, E)
    assert q == want and sum(q) == n and len(q) == E
    assert R.episode_count_targets(n, E).tolist() == want


def test_reference_by_hand():
    """3 envs, 6 steps, quotas [1, 0, 2].
    step 1: env 1 (quota 0) and env 2 finish: only env 2 is logged, return 2 - 1 = 1 over 2 steps.
    step 2: envs 0 and 2 finish in one step: env 0's 1 + 0.5 + 0.25 = 1.75 over 3 steps is appended before
            env 2's 3.0 over 1 step (ascending env index).  Every quota is met.
    steps 3-5: env 0 finishes at step 4, env 2 at step 5, env 1 at step 3: nothing more is logged."""
    rew = [[1.0, 0.5, 2.0], [0.5, 0.5, -1.0], [0.25, 1.0, 3.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]
    term = [[0, 0, 0], [0, 1, 0], [1, 0, 1], [0, 0, 0], [1, 0, 0], [0, 0, 0]]
    trunc = [[0, 0, 0], [0, 0, 1], [0, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 1]]
    acc = R.Accounts(3, 3, False, [1, 0, 2])
    left = []
    for t in range(6):
        acc.step(rew[t], term[t], trunc[t])
        left.append(acc.remaining)
    r, n, i = acc.episodes()
    assert r.tolist() == [1.0, 1.75, 3.0] and n.tolist() == [2, 3, 1] and i.tolist() == [2, 0, 2]
    assert left == [3, 2, 0, 0, 0, 0]
    assert acc.episode_counts.tolist() == [1, 0, 2] and acc.total == 3 and acc.steps == 6 and acc.dropped == 0
    s = acc.summary()
    assert s["ep_rew_mean"] == pytest.approx(5.75 / 3, rel=1e-15) and s["ep_len_mean"] == 2.0
    # np.std, ddof 0: sqrt(mean(x^2) - mean^2)
    assert s["ep_rew_std"] == pytest.approx(np.sqrt((1 + 1.75 ** 2 + 9) / 3 - (5.75 / 3) ** 2), rel=1e-12)
    assert s["ep_len_std"] == pytest.approx(np.sqrt(2 / 3), rel=1e-12)
    assert (s["ep_rew_min"], s["ep_rew_max"], s["n"], s["total"]) == (1.0, 3.0, 3.0, 3.0)
    # evaluate_policy's own loop: 3 episodes on 3 envs are targets [1, 1, 1].  Step 1 logs env 1 (0.5 + 0.5 over
    # 2 steps) and env 2 (1.0 over 2), step 2 logs env 0 (1.75 over 3) and skips env 2 (target met); the loop
    # stops there, after 3 steps
    er, el, steps = R.evaluate_policy_accounts(lambda t: (rew[t], term[t], trunc[t]), 3, 3)
    assert (er, el, steps) == ([1.0, 1.0, 1.75], [2, 2, 3], 3)
    # the Monitor window: every finished episode, the last two of them
    win = R.Accounts(3, 2, True)
    for t in range(6):
        win.step(rew[t], term[t], trunc[t])
    # in order: (t1: e1 1.0/2, e2 1.0/2) (t2: e0 1.75/3, e2 3.0/1) (t3: e1 2.0/2) (t4: e0 2.0/2) (t5: e2 3.0/3)
    assert win.total == 7
    assert [e.tolist() for e in win.episodes()] == [[2.0, 3.0], [2, 3], [0, 2]]
    assert np.isnan(R.Accounts(2, 4, True).summary()["ep_rew_mean"])           # safe_mean of nothing


def test_stream_totals():
    """the constructed stream of the GPU tests: the totals and the largest step the issue states"""
    for E, total, most in ((1, 12, 1), (63, 360, 45), (64, 372, 46), (65, 380, 47), (1024, 5860, 732), (1025, 5866, 733),
                           (2049, 11714, 1464)):
        rew, term, trunc = R.stream(24, E)
        done = term | trunc
        assert not (term & trunc).any() and rew.dtype == np.float32
        assert (int(done.sum()), int(done.sum(1).max())) == (total, most)
        assert np.array_equal(rew.astype(np.float64) * 8, np.round(rew.astype(np.float64) * 8))   # multiples of 1/8


class _Learner:
    def state_dict(self):
        return {"log_std": torch.zeros(1)}


def test_evaluator_schedule_best_and_threshold(monkeypatch, tmp_path):
    """means 1, 3, 2, 5 against a threshold of 4: best 1 -> 3 -> 3 -> 5, continue True, True, True, False,
    the best parameters written three times, evaluations.npz under SB3's keys"""
    means = iter([1.0, 3.0, 2.0, 5.0])
    calls = []

    def fake(policy, env, n_eval_episodes, deterministic, return_episode_rewards=False):
        m = next(means)
        calls.append((n_eval_episodes, deterministic, return_episode_rewards))
        return [m - 0.5, m + 0.5, m], [10, 12, 11]
    monkeypatch.setattr(evaluation, "evaluate_policy", fake)
    saves = []
    real_save = torch.save
    monkeypatch.setattr(torch, "save", lambda obj, path: (saves.append(path), real_save(obj, path)))
    best, logs = str(tmp_path / "best" / "policy.pth"), str(tmp_path / "logs")
    ev = evaluation.Evaluator(_stub_env(), object(), n_eval_episodes=3, eval_freq=1000, reward_threshold=4.0,
                              best_path=best, log_path=logs)
    out, bests, evaluated = [], [], []
    # rollouts of 256 steps: n_calls crosses 1000 at 1024, 2000 at 2048, 3000 at 3072, 4000 at 4096
    for k in range(1, 17):
        go = ev.on_rollout(k * 256 * 8, k * 256, _Learner())
        if ev.evaluated:
            out.append(go)
            bests.append(ev.best_mean_reward)
            evaluated.append(k * 256)
        else:
            assert go is True
        if not go:
            break
    assert evaluated == [1024, 2048, 3072, 4096]          # the first rollout boundary after each multiple
    assert bests == [1.0, 3.0, 3.0, 5.0] and out == [True, True, True, False]
    assert saves == [best] * 3 and set(torch.load(best)) == {"log_std"}
    assert calls == [(3, True, True)] * 4
    z = np.load(os.path.join(logs, "evaluations.npz"))
    assert set(z.files) == {"timesteps", "results", "ep_lengths"}
    assert z["timesteps"].tolist() == [1024 * 8, 2048 * 8, 3072 * 8, 4096 * 8]
    assert z["results"].shape == (4, 3) and z["ep_lengths"].shape == (4, 3)
    assert z["results"][:, 2].tolist() == [1.0, 3.0, 2.0, 5.0]
    # no threshold: never stops; a rollout longer than eval_freq evaluates once per call
    monkeypatch.setattr(evaluation, "evaluate_policy", lambda *a, **k: ([9.0], [1]))
    ev2 = evaluation.Evaluator(_stub_env(), object(), n_eval_episodes=1, eval_freq=100)
    assert [ev2.on_rollout(k * 256, k * 256) for k in (1, 2)] == [True, True] and ev2.n_evaluations == 2
    assert ev2.on_rollout(568, 568) is True and ev2.n_evaluations == 2       # 512 -> 568: no multiple of 100 crossed
