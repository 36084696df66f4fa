"""On-device policy path, CPU part: the oracle's RLController transforms against the
reference's own outputs (tests/golden/policy_golden.npz), the oracle actor against a torch
fp32 forward, and the SB3 zip loader.  The kernel itself: tests/test_policy_gpu.py."""
import io
import json
import os
import zipfile

import numpy as np
import pytest
import torch

from oracle import policy as OP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "policy_golden.npz"))
ZIPS = ("example_RL_model", "twogates")


def weights(name):
    return [G[f"{name}_w{i}"] for i in range(6)], bool(G[f"{name}_relu"])


def test_rlcontroller_transforms_match_reference():
    obs, a = G["pol_obs"], G["pol_agent_act"]
    np.testing.assert_array_equal(OP.rl_transform(a, obs, "relative"), G["pol_relative"])
    np.testing.assert_array_equal(OP.rl_transform(a, obs, "absolute"), G["pol_absolute"])
    assert np.abs(G["pol_relative"][:, 3]).max() <= np.pi      # map2pi range, incl. the +-pi edges


@pytest.mark.parametrize("name", ZIPS)
def test_actor_matches_torch_fp32(name):
    w, relu = weights(name)
    assert w[0].shape[1] == 49 and w[4].shape[0] == 4
    assert relu == (name == "twogates")                        # policy_kwargs activation_fn
    x = G["pol_obs"]
    net = torch.nn.Sequential(torch.nn.Linear(49, w[0].shape[0]), torch.nn.ReLU() if relu else torch.nn.Tanh(),
                              torch.nn.Linear(w[2].shape[1], w[2].shape[0]), torch.nn.ReLU() if relu else torch.nn.Tanh(),
                              torch.nn.Linear(w[4].shape[1], 4))
    with torch.no_grad():
        for i, lin in enumerate((net[0], net[2], net[4])):
            lin.weight.copy_(torch.from_numpy(w[2 * i])); lin.bias.copy_(torch.from_numpy(w[2 * i + 1]))
        ref = net(torch.from_numpy(x.astype(np.float32))).double().numpy()
    np.testing.assert_allclose(OP.actor_mean(w, x, relu), ref, rtol=1e-5, atol=1e-5)
    p = OP.sb3_predict(w, x, relu)
    assert p.min() >= -1 and p.max() <= 1


def _sb3_zip(path, name):
    """a model zip in the layout SB3's save() writes and the reference's user_controller zips have:
    `policy.pth` = torch.save of the policy's state dict (the stored actor weights of `name`, beside
    critic and log_std entries that the actor loader has to pass over), `data` = the JSON of the
    constructor arguments (policy_kwargs.activation_fn as the class's repr; absent for the default
    Tanh policy, as in example_RL_model.zip)"""
    from gym_pybullet_adrp_amd.policy import ACTOR_KEYS, CRITIC_KEYS
    w, relu = weights(name)
    sd = {k: torch.from_numpy(np.array(w[i])) for i, k in enumerate(ACTOR_KEYS)}
    h = w[2].shape[0]
    rng = np.random.default_rng(5)
    for k, shape in zip(CRITIC_KEYS, ((w[0].shape[0], 49), (w[0].shape[0],), (h, w[0].shape[0]), (h,), (1, h), (1,), (4,))):
        sd[k] = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    buf = io.BytesIO()
    torch.save(sd, buf)
    data = {"policy_class": {":type:": "<class 'abc.ABCMeta'>", "__module__": "stable_baselines3.common.policies"},
            "verbose": 0, "policy_kwargs": {}}
    if relu:
        data["policy_kwargs"] = {":type:": "<class 'dict'>", "net_arch": [{"pi": [h, h], "vf": [h, h]}],
                                 "activation_fn": "<class 'torch.nn.modules.activation.ReLU'>"}
    with zipfile.ZipFile(path, "w") as zf:
        zf.writestr("data", json.dumps(data))
        zf.writestr("policy.pth", buf.getvalue())
        zf.writestr("_stable_baselines3_version", "2.3.2")
    return path


@pytest.mark.parametrize("name", ZIPS)
def test_sb3_zip_loader(name, tmp_path):
    from gym_pybullet_adrp_amd.policy import ACTOR_KEYS, load_sb3_zip
    w, act = load_sb3_zip(_sb3_zip(str(tmp_path / f"{name}.zip"), name))
    for i, k in enumerate(ACTOR_KEYS):
        np.testing.assert_array_equal(w[k], G[f"{name}_w{i}"])
    assert act == ("relu" if name == "twogates" else "tanh")
