"""Wide on-device policy kernels (csrc/policy_kernel.h policy_wide_kernel / policy_sample_wide_kernel:
in_dim <= 576, act_dim <= 32) against the float64 oracle (oracle/policy.py).  Needs an MI355X: -m gpu.

Nets and inputs: tests/test_policy_wide.py random_net / random_obs (pre-activations O(1)).  A float32
sequential forward of such a net stays below 1.5e-6 absolute of the float64 one up to
576 -> 64 -> 64 -> 32, so the narrow kernels' bars hold unchanged with a factor above 10: action 2e-5
absolute, value 2e-5 max(1, |v|), log-prob 1e-4 max(1, |lp|), the Gaussian draws bit for bit."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd.policy import ACTOR_KEYS, CRITIC_KEYS, DevicePolicy  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import policy as OP  # noqa: E402
from tests.test_policy import weights  # noqa: E402
from tests.test_policy_wide import actor, critic, random_net, random_obs  # noqa: E402

TOL = 2e-5
SHAPES = [(72, 64, 64, 4), (65, 16, 16, 5), (81, 16, 128, 3), (144, 64, 64, 8), (216, 128, 32, 12), (576, 64, 64, 32)]


def wide_eps(rows, seed, counter, act_dim):
    """the wide sample kernel's standard normals: one Philox4x32-10 block per (row, output quad q),
    counter {row, counter, 0x504f4c00, q}; columns 4q .. 4q + 3 are the Box-Muller of its word pairs"""
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    nq = -(-act_dim // 4)
    out = np.zeros((rows, 4 * nq), np.float32)
    for r in range(rows):
        for q in range(nq):
            x = O.philox([r, counter & 0xFFFFFFFF, 0x504F4C00, q], key)
            out[r, 4 * q:4 * q + 2] = O.normal_pair(x[0], x[1])
            out[r, 4 * q + 2:4 * q + 4] = O.normal_pair(x[2], x[3])
    return out[:, :act_dim]


@pytest.mark.parametrize("relu", [False, True], ids=["tanh", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_wide_act_matches_oracle(shape, relu):
    rng = np.random.default_rng(sum(shape))
    wd = random_net(rng, *shape)
    pol = DevicePolicy(wd, "relu" if relu else "tanh", 0, "raw")
    assert pol.in_dim == shape[0] and pol.act_dim == shape[3]
    for rows in (1, 15, 17, 64, 1000):
        x = random_obs(rng, (rows, shape[0]))
        got = pol.act(torch.from_numpy(x).cuda())
        assert got.shape == (rows, shape[3])
        ref = OP.sb3_predict(actor(wd), x, relu)
        err = np.abs(got.cpu().numpy() - ref).max()
        print(f"{shape} relu={relu} rows={rows}: max err {err:.3e}")
        assert err <= TOL, f"rows={rows}: max err {err:.3e}"
    pol.close()


def test_two_output_tiles_on_one_wave_and_raw_act_of_a_narrow_policy():
    """two paths the shapes above do not take: 16 / 16 hidden units give the block one wave per net, which
    then computes both output tiles of a 20-output policy in turn (act and sample); and a RAW act() of a
    narrow 27 -> 1 policy (learn.py's ONE_D_RPM hover actor), which the wide kernel serves from the narrow
    blob because the narrow kernel stores float4 rows"""
    rng = np.random.default_rng(21)
    wd = random_net(rng, 100, 16, 16, 20)
    pol = DevicePolicy(wd, "tanh", 0, "raw")
    x = random_obs(rng, (333, 100))
    xd = torch.from_numpy(x).cuda()
    assert np.abs(pol.act(xd).cpu().numpy() - OP.sb3_predict(actor(wd), x, False)).max() <= TOL
    eps = torch.empty((333, 20), device="cuda")
    _, act, val, lp = pol.sample(xd, 3, 4, eps=eps)
    e_ref = wide_eps(333, 3, 4, 20)
    np.testing.assert_array_equal(eps.cpu().numpy(), e_ref)
    a_ref, v_ref, lp_ref = OP.sample(actor(wd), critic(wd), x, False, e_ref)
    assert np.abs(act.cpu().numpy() - a_ref).max() <= TOL
    assert np.abs(val.cpu().numpy() - v_ref).max() <= TOL * max(1.0, np.abs(v_ref).max())
    assert np.abs(lp.cpu().numpy() - lp_ref).max() <= 1e-4 * max(1.0, np.abs(lp_ref).max())
    pol.close()
    wd = random_net(rng, 27, 64, 64, 1)
    pol = DevicePolicy(wd, "tanh", 0, "raw")
    x = random_obs(rng, (100, 27))
    got = pol.act(torch.from_numpy(x).cuda())
    assert got.shape == (100, 1)
    assert np.abs(got.cpu().numpy() - OP.sb3_predict(actor(wd), x, False)).max() <= TOL
    pol.close()


def test_wide_act_obs_stride():
    """a 144-wide policy on 160-wide rows reads the first 144 columns of each (the rest non-finite)"""
    rng = np.random.default_rng(4)
    wd = random_net(rng, 144, 64, 64, 8)
    pol = DevicePolicy(wd, "tanh", 0, "raw")
    x = random_obs(rng, (7, 37, 160))
    x[..., 144:] = np.nan
    got = pol.act(torch.from_numpy(x).cuda()).cpu().numpy()
    assert got.shape == (7, 37, 8)
    err = np.abs(got - OP.sb3_predict(actor(wd), x[..., :144], False)).max()
    print(f"stride 160: max err {err:.3e}")
    assert err <= TOL
    pol.close()


def test_wide_relative_whole_compete_row():
    """RLController's RELATIVE transform from a policy that reads a whole 4-drone COMPETE row (67 floats)"""
    rng = np.random.default_rng(6)
    wd = random_net(rng, 67, 64, 64, 4)
    pol = DevicePolicy(wd, "tanh", 0, "relative")
    x = random_obs(rng, (250, 4, 67))
    got = pol.act(torch.from_numpy(x).cuda()).cpu().numpy().reshape(-1, 4)
    xx = x.reshape(-1, 67)
    ref = OP.rl_transform(OP.sb3_predict(actor(wd), xx, False), xx, "relative")
    err = np.abs(got - ref)
    err[:, 3] = np.abs(np.angle(np.exp(1j * (got[:, 3] - ref[:, 3]))))   # yaw on the circle (the +-pi seam)
    print(f"relative 67 -> 4: max err {err.max():.3e}")
    assert err.max() <= TOL
    pol.close()


@pytest.mark.parametrize("shape", [(72, 64, 64, 4), (144, 64, 64, 8), (81, 16, 128, 3), (576, 64, 64, 32)],
                         ids=lambda s: "-".join(map(str, s)))
def test_wide_sample_matches_sb3_forward(shape):
    rng = np.random.default_rng(sum(shape) + 1)
    wd = random_net(rng, *shape)
    pol = DevicePolicy(wd, "tanh", 0, "raw")
    assert pol.has_critic
    A, seed = shape[3], 2024
    w, v = actor(wd), critic(wd)
    for rows, counter in ((1, 0), (17, 3), (1000, 77)):
        x = random_obs(rng, (rows, shape[0]))
        eps = torch.empty((rows, A), device="cuda")
        env_act, act, val, lp = pol.sample(torch.from_numpy(x).cuda(), seed, counter, eps=eps)
        torch.cuda.synchronize()
        e_ref = wide_eps(rows, seed, counter, A)
        np.testing.assert_array_equal(eps.cpu().numpy(), e_ref)                 # the draws, bit for bit
        np.testing.assert_array_equal(e_ref[:, :4], OP.policy_eps(rows, seed, counter, min(A, 4)))   # quad 0
        a_ref, v_ref, lp_ref = OP.sample(w, v, x, False, e_ref)
        ea, ev, el = (np.abs(act.cpu().numpy() - a_ref).max(), np.abs(val.cpu().numpy() - v_ref).max(),
                      np.abs(lp.cpu().numpy() - lp_ref).max())
        print(f"{shape} rows={rows}: action {ea:.3e} value {ev:.3e} log_prob {el:.3e}")
        assert act.shape == (rows, A) and env_act.shape == (rows, A)
        assert ea <= TOL
        assert ev <= TOL * max(1.0, np.abs(v_ref).max())
        assert el <= 1e-4 * max(1.0, np.abs(lp_ref).max())
        assert np.abs(env_act.cpu().numpy() - np.clip(a_ref, -1, 1)).max() <= TOL
        np.testing.assert_array_equal(env_act.cpu().numpy(), np.clip(act.cpu().numpy(), -1, 1))
    xd = torch.from_numpy(x[:64]).cuda()                   # the draws follow the counter
    a1 = pol.sample(xd, seed, 1)[1].cpu().numpy()
    a2 = pol.sample(xd, seed, 2)[1].cpu().numpy()
    assert not np.array_equal(a1, a2)
    pol.close()


def test_forced_wide_gives_the_narrow_bits(monkeypatch):
    """the reference's example_RL_model (49 -> 64 -> 64 -> 4) on the narrow kernels and, created under
    ADRP_POLICY_WIDE=1, on the wide ones.  The wide kernel keeps the narrow accumulation order (even /
    odd k-steps on two chains, a0 + a1 + b) and quad 0's Philox stream, so the actions
    and the draws are the same bits."""
    w, relu = weights("example_RL_model")
    c = np.load(os.path.join(os.path.dirname(__file__), "golden", "critic_golden.npz"))
    wd = dict(zip(ACTOR_KEYS, w))
    wd.update(zip(CRITIC_KEYS, [c[f"example_RL_model_v{i}"] for i in range(7)]))
    rng = np.random.default_rng(12)
    x = torch.from_numpy(random_obs(rng, (1000, 49))).cuda()
    out = {}
    for mode in ("raw", "relative"):
        monkeypatch.delenv("ADRP_POLICY_WIDE", raising=False)
        narrow = DevicePolicy(wd, "relu" if relu else "tanh", 0, mode)
        monkeypatch.setenv("ADRP_POLICY_WIDE", "1")
        wide = DevicePolicy(wd, "relu" if relu else "tanh", 0, mode)
        monkeypatch.delenv("ADRP_POLICY_WIDE", raising=False)
        for name, pol in (("narrow", narrow), ("wide", wide)):
            eps = torch.empty((1000, 4), device="cuda")
            s = pol.sample(x, 5, 9, eps=eps)
            out[name] = [pol.act(x).cpu().numpy(), eps.cpu().numpy()] + [t.cpu().numpy() for t in s]
            pol.close()
        np.testing.assert_array_equal(out["wide"][0], out["narrow"][0])        # act(): bit-identical
        np.testing.assert_array_equal(out["wide"][1], out["narrow"][1])        # eps: bit-identical
        # sample(): the same forward, the same draws and the same log-prob sum (one live quad): the same bits
        for k, name in enumerate(("env_act", "action", "value", "log_prob"), 2):
            d = np.abs(out["wide"][k] - out["narrow"][k]).max()
            print(f"{mode} sample {name}: max |wide - narrow| = {d:.3e}")
            np.testing.assert_array_equal(out["wide"][k], out["narrow"][k], err_msg=name)


def test_wide_policy_and_multihover_step_in_one_graph():
    """policy.act (144 -> 8, the joint two-drone agent) + the MultiHoverAviary step in one linear HIP graph,
    replayed 20 times: the action fed to the last step is the oracle's forward of that step's obs"""
    from gym_pybullet_adrp_amd.envs.multihover import MultiHoverAviary
    E = 256
    env = MultiHoverAviary(num_drones=2, num_envs=E, seed=5, init_noise={"xyz": 0.1, "rpy": 0.1})
    wd = random_net(np.random.default_rng(8), 144, 64, 64, 8)
    pol = DevicePolicy(wd, "tanh", 0, "raw")
    obs, _ = env.reset()
    assert obs.shape == (E, 2, 72)
    act = torch.empty((E, 2, 4), device=obs.device)
    seen = torch.empty((E, 144), device=obs.device)

    def one():
        seen.copy_(env._obs.view(E, 144))
        pol.act(seen, out=act)
        env.step(act)
    one()                                                  # eager warm-up
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        one()                                              # warm the side stream
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            one()
    for _ in range(20):
        g.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(env._obs).all() and torch.isfinite(act).all()
    ref = OP.sb3_predict(actor(wd), seen.cpu().numpy(), False)
    err = np.abs(act.cpu().numpy().reshape(E, 8) - ref).max()
    print(f"graph: max err {err:.3e}")
    assert err <= TOL
    env.close()
    pol.close()
