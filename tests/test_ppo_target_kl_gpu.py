"""The target_kl latch and the rate schedules of ``PPOLearner`` on the device (csrc/ppo_kernel.h, csrc/ppo.hip,
include/adrp_train.h).  Needs an MI355X: -m gpu.

Yardsticks: ``train_loop_kl`` (tests/ppo_train_reference.py: SB3's loop with its stop, float64) for where the stop
trips and for the final parameters, within tests/test_ppo_update_gpu.py's trajectory bar; and a twin learner that
applies minibatches 0..k*-1 through manual ``update`` calls, for everything the stop must leave bit for bit.
The cases and their conditions are asserted on the reference alone in tests/test_ppo_target_kl_abi.py."""
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd.policy import DevicePolicy  # noqa: E402
from gym_pybullet_adrp_amd.ppo import PPOLearner, linear_schedule  # noqa: E402
from tests import ppo_reference as R  # noqa: E402
from tests import ppo_train_reference as T  # noqa: E402
from tests.test_ppo_update_gpu import bar  # noqa: E402

CASES = range(len(T.CASES))
IDS = ["-".join(map(str, c.shape)) + "-" + c.activation for c in T.CASES]


def collector(c):
    dev = [torch.from_numpy(np.ascontiguousarray(b)).cuda() for b in c.buf]
    return SimpleNamespace(T=c.c.rows, E=1, obs=dev[0], actions=dev[1], values=dev[2], log_probs=dev[3], advantages=dev[4],
                           returns=dev[5])


def flat_of(col):
    n = col.T * col.E
    return (col.obs.view(n, -1), col.actions.view(n, -1), col.values.view(n), col.log_probs.view(n), col.advantages.view(n),
            col.returns.view(n))


class Pair:
    """a policy and its learner, closed in the right order"""

    def __init__(self, c, target_kl=None, **kw):
        kw = dict(dict(learning_rate=c.c.lr, n_epochs=c.c.epochs, batch_size=c.c.batch), **kw)
        self.pol = DevicePolicy(c.w, c.c.activation, 0, "raw")
        self.learner = PPOLearner(self.pol, **kw)
        assert self.learner.target_kl is None                 # a new learner has no stop
        self.learner.set_target_kl(target_kl)                 # (the constructor's keyword stays refused)

    def state(self):
        osd = self.learner.optimizer_state_dict()
        return self.learner.state_dict(), osd["exp_avg"], osd["exp_avg_sq"], osd["step"]

    def output(self, c):
        x = torch.from_numpy(np.random.default_rng(99).normal(size=(40, c.c.shape[0])).astype(np.float32)).cuda()
        return self.pol.act(x).clone()

    def close(self):
        self.learner.close()
        self.pol.close()


def same_state(a, b):
    for k in R.KEYS:
        for i in range(3):
            assert torch.equal(a[i][k], b[i][k]), (k, i)
    assert a[3] == b[3]


def minibatch(c, perms, j):
    e, k = divmod(j, c.nmb)
    return perms[e, k * c.c.batch:(k + 1) * c.c.batch].contiguous()


@pytest.mark.parametrize("i", CASES, ids=IDS)
def test_the_stop_trips_where_the_reference_trips_and_leaves_the_rest_untouched(i):
    c = T.case(i)
    col, perms = collector(c), torch.from_numpy(c.perms).cuda()
    a = Pair(c, target_kl=c.target_kl)
    stats = a.learner.train(col, permutations=perms)
    torch.cuda.synchronize()
    assert stats.shape == (c.c.epochs, c.nmb, 5)
    flat = stats.view(c.n, 5)
    kl = flat[:, 3].cpu().double().numpy()
    print(f"case {i}: device KL {['%.3e' % x for x in kl]} reference {['%.3e' % x for x in c.kl64[:c.k + 1]]} k* {c.k}")
    # the device trips at the reference's k*
    assert a.learner.stop_state.cpu().tolist() == [1, c.k]
    e, k = divmod(c.k, c.nmb)
    assert a.learner.stop_info() == {"stopped": True, "updates": c.k, "epoch": e, "minibatch": k}
    # the twin: minibatches 0 .. k* - 1 by manual update calls
    b = Pair(c)
    tw = torch.zeros((c.k + 1, 5), device="cuda")
    for j in range(c.k):
        b.learner.update(*flat_of(col), minibatch(c, perms, j), stats=tw[j])
    torch.cuda.synchronize()
    got, want = a.state(), b.state()
    same_state(got, want)
    assert got[3] == c.k
    assert torch.equal(a.output(c), b.output(c))
    # the final parameters against SB3's loop with its stop, float64, within the trajectory bar
    p64, _, trip = T.train_loop_kl(c.w, c.buf, c.perms, c.c.batch, c.cfg, c.relu, torch.float64, target_kl=c.target_kl)
    p32, _, _ = T.train_loop_kl(c.w, c.buf, c.perms, c.c.batch, c.cfg, c.relu, torch.float32, target_kl=c.target_kl)
    assert trip == c.k
    e32 = R.tensor_errors(p32, p64)
    err = R.tensor_errors({key: v.cpu() for key, v in got[0].items()}, p64)
    print(f"case {i}: trajectory error {max(err.values()):.3e}, e32 {max(e32.values()):.3e}")
    for key in R.KEYS:
        assert err[key] <= bar(e32[key]), (key, err[key], e32[key])
    # the statistics: rows < k* the twin's, row k* what the twin reports when it then runs minibatch k*, the rest NaN
    b.learner.update(*flat_of(col), minibatch(c, perms, c.k), stats=tw[c.k])
    torch.cuda.synchronize()
    assert torch.equal(flat[:c.k + 1], tw)
    assert bool(torch.isnan(flat[c.k + 1:]).all()) and flat[c.k + 1:].numel() > 0
    assert kl[c.k] > c.thr > kl[:c.k].max()
    # a second train() clears the latch and moves the parameters (the target far away: it runs to the end)
    a.learner.set_target_kl(1e9)
    a.learner.train(col, permutations=perms)
    torch.cuda.synchronize()
    assert a.learner.stop_state.cpu().tolist() == [0, c.n]
    assert a.learner.stop_info() == {"stopped": False, "updates": c.n, "epoch": None, "minibatch": None}
    again = a.state()
    assert again[3] == c.k + c.n
    for key in R.KEYS:
        assert not torch.equal(again[0][key], got[0][key]), key
    a.close()
    b.close()


@pytest.mark.parametrize("i", CASES, ids=IDS)
def test_a_target_that_is_never_reached_gives_the_bits_of_none(i):
    c = T.case(i)
    col, perms = collector(c), torch.from_numpy(c.perms).cuda()
    out = []
    for target in (None, 1e9):
        a = Pair(c, target_kl=target)
        stats = a.learner.train(col, permutations=perms)
        torch.cuda.synchronize()
        out.append((a.state(), stats.clone(), a.learner.stop_state.cpu().tolist()))
        a.close()
    same_state(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1]) and bool(torch.isfinite(out[1][1]).all())
    assert out[0][2] == out[1][2] == [0, c.n]
    # and the setter takes effect on a learner that has trained without a target, and None switches it off again
    a = Pair(c)
    a.learner.train(col, permutations=perms)
    a.learner.load_state_dict({k: torch.from_numpy(c.w[k]) for k in R.KEYS})
    zero = {k: torch.zeros(c.w[k].shape) for k in R.KEYS}
    a.learner.load_optimizer_state_dict({"exp_avg": zero, "exp_avg_sq": zero, "step": 0})
    a.learner.set_target_kl(c.target_kl)
    a.learner.train(col, permutations=perms)
    torch.cuda.synchronize()
    assert a.learner.stop_state.cpu().tolist() == [1, c.k] and a.learner.target_kl == c.target_kl
    a.learner.set_target_kl(None)
    stats = a.learner.train(col, permutations=perms)
    torch.cuda.synchronize()
    assert a.learner.stop_state.cpu().tolist() == [0, c.n] and bool(torch.isfinite(stats).all())
    a.close()


def test_a_graph_of_train_begin_and_updates_gives_the_eager_bits():
    """one HIP graph: train_begin and the first k* + 3 updates on one stream; the three behind the trip are no-ops"""
    c = T.case(0)
    col, perms = collector(c), torch.from_numpy(c.perms).cuda()
    n = c.k + 3
    assert n <= c.n
    idx = [minibatch(c, perms, j) for j in range(n)]
    results = []
    for graphed in (False, True):
        a = Pair(c, target_kl=c.target_kl)
        stats = torch.full((n, 5), float("nan"), device="cuda")

        def issue():
            a.learner.train_begin()
            for j in range(n):
                a.learner.update(*flat_of(col), idx[j], stats=stats[j])
            a.learner.read_stop_state()

        if graphed:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                issue()
            assert a.learner.optimizer_state_dict()["step"] == 0          # captured, not run
            graph.replay()
        else:
            issue()
        torch.cuda.synchronize()
        results.append((a.state(), stats.clone(), a.learner.stop_state.cpu().tolist()))
        a.close()
    same_state(results[0][0], results[1][0])
    assert results[0][2] == results[1][2] == [1, c.k]
    assert torch.equal(results[0][1].view(torch.int32), results[1][1].view(torch.int32))
    assert bool(torch.isnan(results[1][1][c.k + 1:]).all()) and bool(torch.isfinite(results[1][1][:c.k + 1]).all())


def test_schedules_are_evaluated_at_progress_remaining():
    """train(col, progress_remaining=0.25) with linear_schedule callables equals a learner built with the constants
    the callables return there"""
    c = T.case(0)
    col, perms = collector(c), torch.from_numpy(c.perms).cuda()
    lr, clip, clip_vf = linear_schedule(4e-3, 1e-3, 0.5), linear_schedule(0.3, 0.1), linear_schedule(0.4)
    assert (lr(0.25), clip(0.25), clip_vf(0.25)) == (1e-3, 0.3 + 0.75 * (0.1 - 0.3), 0.4 + 0.75 * (0.0 - 0.4))
    a = Pair(c, learning_rate=lr, clip_range=clip, clip_range_vf=clip_vf)
    b = Pair(c, learning_rate=lr(0.25), clip_range=clip(0.25), clip_range_vf=clip_vf(0.25))
    d = Pair(c, learning_rate=lr(1.0), clip_range=clip(1.0), clip_range_vf=clip_vf(1.0))
    sa = a.learner.train(col, permutations=perms, progress_remaining=0.25)
    sb = b.learner.train(col, permutations=perms)
    sd = d.learner.train(col, permutations=perms)
    torch.cuda.synchronize()
    same_state(a.state(), b.state())
    assert torch.equal(sa, sb)
    assert (a.learner.cfg.learning_rate, a.learner.cfg.clip_range, a.learner.cfg.clip_range_vf) == (lr(0.25), clip(0.25), clip_vf(0.25))
    # not vacuous: the rates at the start of training give other parameters and other clip fractions
    assert not torch.equal(a.state()[0][R.KEYS[0]], d.state()[0][R.KEYS[0]]) and not torch.equal(sa, sd)
    for x in (a, b, d):
        x.close()


def test_refusals_behind_a_live_handle():
    c = T.case(0)
    a = Pair(c)
    lib, h = a.learner.lib, a.learner.h
    before = a.state()
    for call, word in ((lambda: lib.adrp_ppo_set_target_kl(h, float("nan")), "adrp_ppo_set_target_kl: target_kl is NaN"),
                       (lambda: lib.adrp_ppo_set_rates(h, 0.0, 0.2, -1.0), "adrp_ppo_set_rates: learning_rate"),
                       (lambda: lib.adrp_ppo_set_rates(h, 3e-4, -0.1, -1.0), "adrp_ppo_set_rates: clip_range"),
                       (lambda: lib.adrp_ppo_stop_state(h, None, None), "adrp_ppo_stop_state: out_dev2 is NULL")):
        assert call() != 0
        assert lib.adrp_last_error(None).decode().startswith(word)
    with pytest.raises(ValueError, match="learning_rate"):
        a.learner.set_rates(-1.0, 0.2)
    for bad in (float("nan"), -0.01):
        with pytest.raises(ValueError, match="target_kl"):
            a.learner.set_target_kl(bad)
    assert a.learner.target_kl is None
    same_state(before, a.state())
    a.close()
