"""On-device PPO update (csrc/ppo_kernel.h, gym_pybullet_adrp_amd/ppo.py) against the float64 torch
restatement of SB3 2.3.2 PPO.train() in tests/ppo_reference.py.  Needs an MI355X: -m gpu.

The bar of the gradient / statistics / trajectory tests is not a constant: torch's own float32
autograd of the same loss on the CPU has error e32 against float64, and the kernel (another f32
evaluation in another summation order, with a branch-free tanh of ~1e-7 absolute error) must stay
within 4 max(e32, 2e-5); 2e-5 is the actor's f32-MFMA bar (tests/test_rollout_gpu.py TOL), the floor
where e32 happens to be tiny.  Error of a tensor: ||g - g64|| / max(||g64||, 1e-3 ||all g64||).

Measured on MI355X (profiles/ppo_update.json holds every figure): the largest kernel error over
the 15 gradient cases is 3.1e-6 (576-16-16-32) where torch's float32 autograd has 3.6e-6, against a bar
of at least 8e-5; the trajectories end 2.4e-7 / 3.2e-7 from the float64 loop (torch float32: 2.5e-7 / 2.9e-7)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd.policy import DevicePolicy  # noqa: E402
from gym_pybullet_adrp_amd.ppo import PPOLearner  # noqa: E402
from tests import ppo_reference as R  # noqa: E402

TOL = 2e-5                      # tests/test_rollout_gpu.py TOL
SHAPES = [                      # in, h1, h2, act, activation, n
    (5, 16, 32, 3, "tanh", 37),          # ragged everything, a partial tile
    (72, 64, 64, 4, "tanh", 64),         # learn.py's default minibatch
    (49, 128, 128, 4, "relu", 200),      # the twogates shape
    (144, 64, 64, 8, "tanh", 1000),      # wide layout, several blocks' partials, a ragged tail
    (576, 16, 16, 32, "tanh", 33),       # the largest in_dim and act_dim
]
SETTINGS = {"defaults": {}, "no_adv_norm": dict(normalize_advantage=False), "vf_clip_entropy": dict(clip_range_vf=0.2, ent_coef=0.01)}


def record(entry):
    """the measured figures, appended to the file ADRP_PPO_ERRORS names (tools: profiles/ppo_update.json)"""
    print(json.dumps(entry))
    path = os.environ.get("ADRP_PPO_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(entry) + "\n")


def bar(e32):
    return 4.0 * max(e32, TOL)


def case(in_dim, h1, h2, act, n, relu, seed):
    """weights, a 4 n-row buffer, a random n-subset idx of it, and the minibatch the subset selects"""
    w = R.make_weights(in_dim, h1, h2, act, seed)
    buf = R.make_buffers(w, 4 * n, relu, seed + 1)
    idx = np.random.default_rng(seed + 2).permutation(4 * n)[:n]
    return w, buf, idx, tuple(b[idx] for b in buf)


def device_update(learner, buf, idx):
    dev = [torch.from_numpy(np.ascontiguousarray(b)).cuda() for b in buf]
    stats = learner.update(*dev, torch.from_numpy(idx).cuda())
    torch.cuda.synchronize()
    return dict(zip(R.STATS, stats.cpu().tolist()))


_cache = {}


def reference(shape, setting):
    """(w, buf, idx, cfg, g64, s64, e32 per tensor, e32 per statistic), computed once per case"""
    key = (shape, setting)
    if key not in _cache:
        in_dim, h1, h2, act, activation, n = shape
        relu = activation == "relu"
        w, buf, idx, batch = case(in_dim, h1, h2, act, n, relu, 100 + SHAPES.index(shape))
        cfg = R.config(**SETTINGS[setting])
        g64, s64, rows = R.gradients(w, batch, cfg, relu, torch.float64)
        # the yardstick first: the batch exercises both branches of the clipped surrogate
        assert float(rows["zero_grad"].double().mean()) >= 0.10
        assert float(rows["unclipped"].double().mean()) >= 0.10
        g32, s32, _ = R.gradients(w, batch, cfg, relu, torch.float32)
        _cache[key] = (w, buf, idx, cfg, g64, s64, R.tensor_errors(g32, g64), R.stat_errors(s32, s64))
    return _cache[key]


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}-{s[3]}-{s[4]}-n{s[5]}")
def test_gradients_and_statistics_match_float64_autograd(shape, setting):
    w, buf, idx, cfg, g64, s64, e32, es32 = reference(shape, setting)
    pol = DevicePolicy(w, shape[4], 0, "raw")
    learner = PPOLearner(pol, **SETTINGS[setting])
    stats = device_update(learner, buf, idx)
    g = learner.gradients()
    err, serr = R.tensor_errors(g, g64), R.stat_errors(stats, s64)
    record(dict(test="gradients", shape=list(shape), setting=setting, e32=max(e32.values()), kernel=max(err.values()),
                e32_stats=max(es32.values()), kernel_stats=max(serr.values())))
    learner.close()
    pol.close()
    for k in R.KEYS:
        assert err[k] <= bar(e32[k]), (k, err[k], e32[k])
    for k in R.STATS:
        assert serr[k] <= bar(es32[k]), (k, stats[k], s64[k], es32[k])


@pytest.mark.parametrize("max_grad_norm, above", [(1e-3, True), (1e6, False)])
def test_clip_and_adam_from_the_kernels_own_gradients(max_grad_norm, above):
    """the float64 clip + Adam step fed the kernel's raw gradients and a non-trivial Adam state"""
    shape = SHAPES[1]
    w, buf, idx, _ = case(*shape[:4], shape[5], False, 7)
    pol = DevicePolicy(w, "tanh", 0, "raw")
    learner = PPOLearner(pol, max_grad_norm=max_grad_norm)
    rng = np.random.default_rng(3)
    m0 = {k: torch.tensor(rng.normal(size=w[k].shape) * 1e-2, dtype=torch.float32) for k in R.KEYS}
    v0 = {k: torch.tensor(rng.random(size=w[k].shape) * 1e-3, dtype=torch.float32) for k in R.KEYS}
    learner.load_optimizer_state_dict({"exp_avg": m0, "exp_avg_sq": v0, "step": 7})
    p0 = {k: v.cpu() for k, v in learner.state_dict().items()}
    for k in R.KEYS:                                  # the learner starts from the policy's weights, bit for bit
        assert np.array_equal(p0[k].numpy(), w[k]), k
    device_update(learner, buf, idx)
    g = {k: v.cpu() for k, v in learner.gradients().items()}
    cfg = R.config(max_grad_norm=max_grad_norm)
    p64, m64, v64, t64, norm = R.clip_adam(p0, g, m0, v0, 7, cfg)
    assert (norm > max_grad_norm) == above
    p1 = learner.state_dict()
    osd = learner.optimizer_state_dict()
    assert osd["step"] == t64 == 8
    for k in R.KEYS:
        d = (p1[k].cpu().double() - p64[k]).abs()
        assert bool((d <= 2.0 ** -22 * p64[k].abs() + 1e-5 * cfg.learning_rate).all()), (k, float(d.max()))
        assert float((p1[k].cpu().double() - p0[k].double()).abs().max()) > 0, k          # and it moved
        np.testing.assert_allclose(osd["exp_avg"][k].cpu().numpy(), m64[k].numpy(), rtol=1e-6, atol=0)
        np.testing.assert_allclose(osd["exp_avg_sq"][k].cpu().numpy(), v64[k].numpy(), rtol=1e-6, atol=0)
    learner.close()
    pol.close()


@pytest.mark.parametrize("shape", [(12, 32, 32, 4, "tanh"), (72, 64, 64, 4, "tanh")], ids=["narrow", "wide"])
def test_trajectory_and_repack(shape):
    """8 updates (100 rows, batch 32 -> slices 32, 32, 32, 4; 2 epochs, given permutations) against the
    float64 loop with torch's clip_grad_norm_ and Adam; then the attached policy itself, through its
    in-place re-packed blobs, must be the float64 forward of the learner's state_dict"""
    in_dim, h1, h2, act, activation = shape
    w = R.make_weights(in_dim, h1, h2, act, 21)
    buf = R.make_buffers(w, 100, False, 22)
    perms = np.stack([np.random.default_rng(23 + e).permutation(100) for e in range(2)])
    cfg = R.config(learning_rate=1e-3)
    p64 = R.train_loop(w, buf, perms, 32, cfg, False, torch.float64)
    p32 = R.train_loop(w, buf, perms, 32, cfg, False, torch.float32)
    e32 = R.tensor_errors(p32, p64)
    pol = DevicePolicy(w, activation, 0, "raw")
    assert bool(pol.lib and pol.has_critic)
    learner = PPOLearner(pol, learning_rate=1e-3, n_epochs=2, batch_size=32)
    dev = [torch.from_numpy(b).cuda() for b in buf]
    col = SimpleNamespace(T=100, E=1, obs=dev[0], actions=dev[1], values=dev[2], log_probs=dev[3], advantages=dev[4],
                          returns=dev[5])
    stats = learner.train(col, permutations=torch.from_numpy(perms))
    torch.cuda.synchronize()
    assert stats.shape == (2, 4, 5) and bool(torch.isfinite(stats).all())
    sd = {k: v.cpu() for k, v in learner.state_dict().items()}
    err = R.tensor_errors(sd, p64)
    record(dict(test="trajectory", shape=list(shape), e32=max(e32.values()), kernel=max(err.values())))
    for k in R.KEYS:
        assert err[k] <= bar(e32[k]), (k, err[k], e32[k])
        assert not np.array_equal(sd[k].numpy(), w[k]), k
    # the policy after the in-place re-pack, on fresh rows
    rng = np.random.default_rng(29)
    x = rng.normal(size=(50, in_dim)).astype(np.float32)
    eps = torch.empty((50, act), device="cuda")
    _, a, val, lp = pol.sample(torch.from_numpy(x).cuda(), 5, 9, eps=eps)
    torch.cuda.synchronize()
    p = {k: v.double() for k, v in sd.items()}
    mean, v_ref = R.forward(p, torch.from_numpy(x).double(), False)
    std = torch.exp(p["log_std"])
    a_ref = mean + std * eps.cpu().double()
    lp_ref, _ = R.log_prob_entropy(p, mean, a.cpu().double())
    assert float((a.cpu().double() - a_ref).abs().max()) <= TOL * max(1.0, float(std.max()))
    assert float((val.cpu().double() - v_ref).abs().max()) <= TOL * max(1.0, float(v_ref.abs().max()))
    assert float((lp.cpu().double() - lp_ref).abs().max()) <= 1e-4 * max(1.0, float(lp_ref.abs().max()))
    # and a policy rebuilt from the state_dict is the same policy, bit for bit
    pol2 = DevicePolicy({k: v.numpy() for k, v in sd.items()}, activation, 0, "raw")
    a2 = pol2.sample(torch.from_numpy(x).cuda(), 5, 9)[1]
    assert torch.equal(a2, a)
    pol2.close()
    learner.close()
    pol.close()


def test_updates_are_deterministic():
    shape = SHAPES[3]
    w, buf, idx, _ = case(*shape[:4], shape[5], False, 31)
    out = []
    for _ in range(2):
        pol = DevicePolicy(w, "tanh", 0, "raw")
        learner = PPOLearner(pol)
        for _ in range(3):
            device_update(learner, buf, idx)
        osd = learner.optimizer_state_dict()
        out.append((learner.state_dict(), osd["exp_avg"], osd["exp_avg_sq"]))
        learner.close()
        pol.close()
    for a, b in zip(out[0], out[1]):
        for k in R.KEYS:
            assert torch.equal(a[k], b[k]), k
    assert not np.array_equal(out[0][0][R.KEYS[0]].cpu().numpy(), w[R.KEYS[0]])


def test_update_in_a_graph_gives_the_eager_bits():
    shape = SHAPES[0]
    w, buf, idx, _ = case(*shape[:4], shape[5], False, 41)
    dev = [torch.from_numpy(np.ascontiguousarray(b)).cuda() for b in buf]
    idx_d = torch.from_numpy(idx).cuda()
    results = []
    for graphed in (False, True):
        pol = DevicePolicy(w, "tanh", 0, "raw")
        learner = PPOLearner(pol)
        stats = torch.zeros(5, device="cuda")
        if graphed:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):                 # one linear chain of four launches
                learner.update(*dev, idx_d, stats=stats)
            assert learner.optimizer_state_dict()["step"] == 0          # captured, not run
            graph.replay()
        else:
            learner.update(*dev, idx_d, stats=stats)
        torch.cuda.synchronize()
        results.append((learner.state_dict(), stats.clone(), learner.optimizer_state_dict()["step"]))
        learner.close()
        pol.close()
    (p_e, s_e, t_e), (p_g, s_g, t_g) = results
    assert t_e == t_g == 1 and torch.equal(s_e, s_g)
    for k in R.KEYS:
        assert torch.equal(p_e[k], p_g[k]), k


def test_refusals_that_need_a_device():
    w = R.make_weights(5, 16, 16, 2, 0)
    actor_only = {k: w[k] for k in R.KEYS[:6]}
    pol = DevicePolicy(actor_only, "tanh", 0, "raw")
    with pytest.raises(ValueError, match="no critic"):
        PPOLearner(pol)
    pol.set_critic(w)
    with pytest.raises(ValueError, match="target_kl"):
        PPOLearner(pol, target_kl=0.01)
    learner = PPOLearner(pol)
    with pytest.raises(ValueError, match="target_kl"):
        learner.train(None, target_kl=0.01)
    learner.close()
    pol.close()


def test_collect_train_collect_hover():
    """learn.py's loop on the device: HoverAviary ONE_D_RPM, collect -> train -> collect"""
    from gym_pybullet_adrp_amd.envs.hover import HoverAviary
    from gym_pybullet_adrp_amd.rollout import RolloutCollector
    from gym_pybullet_adrp_amd.utils.enums import ActionType
    env = HoverAviary(act=ActionType.ONE_D_RPM, num_envs=64, seed=4, initial_xyzs=[0, 0, 1.0])
    w = R.make_weights(27, 64, 64, 1, 51)
    pol = DevicePolicy(w, "tanh", 0, "raw")
    col = RolloutCollector(env, pol, 16, seed=1)
    learner = PPOLearner(pol, n_epochs=2, batch_size=256, seed=3)
    col.reset()
    col.collect()
    values0 = col.values.clone()
    obs0 = col.obs[0].clone()
    stats = learner.train(col)
    torch.cuda.synchronize()
    assert stats.shape == (2, 4, 5) and bool(torch.isfinite(stats).all())
    first = dict(zip(R.STATS, stats[0, 0].cpu().tolist()))
    assert first["clip_fraction"] == 0.0 and abs(first["approx_kl"]) <= 1e-6     # ratio 1 up to the forward's rounding
    sd = learner.state_dict()
    for k in R.KEYS:
        assert not np.array_equal(sd[k].cpu().numpy(), w[k]), k
    # the critic the next rollout samples with is the updated one
    v_new = torch.empty(64, device="cuda")
    col._values_of(obs0, v_new)
    assert not torch.equal(v_new, values0[0])
    col.collect()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(col.values).all()) and not torch.equal(col.values, values0)
    learner.close()
    pol.close()
    env.close()
