"""On-device episode statistics (csrc/episode.hip, evaluation.EpisodeStats) against the numpy restatement
of SB3's accounts (tests/episode_reference.py) on constructed streams, no env involved.  Needs an MI355X:
-m gpu.

Inputs (episode_reference.stream): T = 24 steps, done[t][e] = ((t + 1) % (2 + e % 7) == 0), term on even
envs, trunc on odd ones, rew[t][e] = float32(((31 t + 17 e) % 64 - 20) / 8).  The rewards are multiples of
1/8 below 8 in magnitude: exact in float32, every partial sum exact in float64.  So returns, lengths, envs,
counts and meta are compared bit for bit.  E covers the wave (63 / 64 / 65) and the 1,024-env chunk
(1024 / 1025 / 2049) boundaries of the rank scheme.

adrp_episode_summary: n, min, max, total exact; the mean of n doubles in any summation order is within
n 2^-52 max|x| of numpy's (each of the n - 1 additions and the division rounds by at most 2^-53 of a partial
sum bounded by n max|x|, in both arms), the two-pass std within 4 n 2^-52 max|x|."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd.evaluation import EpisodeStats, episode_count_targets  # noqa: E402
from tests import episode_reference as R  # noqa: E402

T = 24
TOTALS = {1: (12, 1), 63: (360, 45), 64: (372, 46), 65: (380, 47), 1024: (5860, 732), 1025: (5866, 733), 2049: (11714, 1464)}
TENSORS = ("run_return", "run_length", "count", "meta", "log_return", "log_length", "log_env")


def device_stream(E, steps=T):
    rew, term, trunc = R.stream(steps, E)
    return (rew, term, trunc), tuple(torch.from_numpy(a).cuda() for a in (rew, term, trunc))


def run_pair(E, C, ring, quota=None, check_each=None):
    """feed the stream to the device and to the reference -> (EpisodeStats, Accounts)"""
    (rew, term, trunc), (drew, dterm, dtrunc) = device_stream(E)
    st = EpisodeStats(E, 0, capacity=C, ring=ring, quota=quota)
    ref = R.Accounts(E, C, ring, quota)
    for t in range(T):
        st.step(drew[t], dterm[t], dtrunc[t])
        ref.step(rew[t], term[t], trunc[t])
        if check_each is not None:
            check_each(t, st, ref)
    torch.cuda.synchronize()
    return st, ref


def assert_same(st, ref, accumulators=True):
    r, n, e = st.episodes()
    rr, rn, re = ref.episodes()
    assert r.dtype == np.float64 and n.dtype == np.int32 and e.dtype == np.int32
    assert np.array_equal(r.view(np.int64), rr.view(np.int64))        # bit for bit
    assert np.array_equal(n, rn) and np.array_equal(e, re)
    assert st.count.cpu().numpy().tolist() == ref.episode_counts.tolist()
    assert st.meta.cpu().numpy().tolist() == [ref.total, ref.remaining, ref.steps, ref.dropped]
    if accumulators:    # (with a quota the running sums of an env past it are unspecified)
        assert np.array_equal(st.run_return.cpu().numpy().view(np.int64), ref.current_rewards.view(np.int64))
        assert st.run_length.cpu().numpy().tolist() == ref.current_lengths.tolist()


@pytest.mark.parametrize("E", sorted(TOTALS))
def test_ring_window_matches_deque(E):
    """Monitor window of 100: wraps across steps; from E = 1024 one step alone has more than 100 finishers"""
    st, ref = run_pair(E, 100, True)
    total, most = TOTALS[E]
    assert ref.total == total and max(R.stream(T, E)[1].sum(1) + R.stream(T, E)[2].sum(1)) == most
    assert (most > 100) == (E >= 1024) and (total > 100) == (E > 1)
    assert_same(st, ref)
    assert len(st.episodes()[0]) == min(total, 100)


def test_ring_smaller_than_one_step():
    """C = 32 at E = 65: a step with 47 > 32 finishers keeps its last 32, one writer per slot"""
    st, ref = run_pair(65, 32, True)
    assert TOTALS[65][1] == 47 > 32 and ref.total == 380
    assert_same(st, ref)


def test_first_c_episodes_and_dropped():
    st, ref = run_pair(65, 50, False)
    assert ref.total == 380 and ref.dropped == 330
    assert_same(st, ref)
    assert int(st.meta[3]) == 330 and len(st.episodes()[0]) == 50


def test_quota_1300_on_1025_envs():
    """evaluate_policy's targets for 1300 episodes on 1025 envs: all met after 16 steps; the 8 further steps
    leave remaining at 0 and the log as it was"""
    quota = episode_count_targets(1300, 1025)
    snap = {}

    def each(t, st, ref):
        if t == 14:
            assert ref.remaining > 0
        if t == 15:
            torch.cuda.synchronize()
            snap["log"] = [x.clone() for x in (st.log_return, st.log_length, st.log_env, st.count)]
        if t >= 15:
            assert ref.remaining == 0 and int(st.meta[1]) == 0
    st, ref = run_pair(1025, 1300, False, quota, each)
    assert ref.total == 1300 and ref.dropped == 0
    assert_same(st, ref, accumulators=False)
    for a, b in zip(snap["log"], (st.log_return, st.log_length, st.log_env, st.count)):
        assert torch.equal(a, b)
    assert st.count.cpu().numpy().tolist() == quota


def test_quota_with_zero_targets():
    """3 episodes on 5 envs: targets [0, 0, 1, 1, 1]; envs 0 and 1 finish and are never logged"""
    quota = episode_count_targets(3, 5)
    st, ref = run_pair(5, 3, False, quota)
    assert quota == [0, 0, 1, 1, 1] and ref.total == 3
    done = R.stream(T, 5)[1] | R.stream(T, 5)[2]
    assert done[:, 0].any() and done[:, 1].any()
    assert_same(st, ref, accumulators=False)
    assert sorted(st.episodes()[2].tolist()) == [2, 3, 4]


@pytest.mark.parametrize("E, C, ring", [(65, 100, True), (2049, 100, True), (65, 50, False), (1, 100, True)])
def test_summary(E, C, ring):
    st, ref = run_pair(E, C, ring)
    got, want = st.summary(), ref.summary()
    r, n, _ = ref.episodes()
    k = len(r)
    assert k == min(TOTALS[E][0], C) and k > 0
    for key in ("n", "ep_rew_min", "ep_rew_max", "total"):
        assert got[key] == want[key]
    u = 2.0 ** -52
    for mean, std, x in (("ep_rew_mean", "ep_rew_std", r), ("ep_len_mean", "ep_len_std", n.astype(np.float64))):
        big = np.abs(x).max()
        print(f"E={E} C={C} {mean}: |diff| {abs(got[mean] - want[mean]):.3e} (bound {k * u * big:.3e}); "
              f"{std}: |diff| {abs(got[std] - want[std]):.3e} (bound {4 * k * u * big:.3e})")
        assert abs(got[mean] - want[mean]) <= k * u * big
        assert abs(got[std] - want[std]) <= 4 * k * u * big


def test_summary_of_an_empty_log():
    st = EpisodeStats(7, 0, capacity=10, ring=True)
    s = st.summary()
    assert s["n"] == 0 and s["total"] == 0
    assert all(np.isnan(s[k]) for k in ("ep_rew_mean", "ep_len_mean", "ep_rew_std", "ep_len_std"))
    r, n, e = st.episodes()
    assert len(r) == len(n) == len(e) == 0 and len(st.episode_times(30)) == 0


def test_episode_times_and_reset():
    st, ref = run_pair(65, 100, True)
    assert np.array_equal(st.episode_times(25), (ref.episodes()[1] - 1) / 25.0)
    st.reset()
    assert all(int(getattr(st, k).abs().sum()) == 0 for k in TENSORS)


def test_step_validates_its_inputs():
    st = EpisodeStats(8, 0)
    rew, z = torch.zeros(8, device="cuda"), torch.zeros(8, dtype=torch.bool, device="cuda")
    for bad in ((rew.double(), z, z), (rew[:7], z, z), (rew, z.float(), z), (rew, z, z[:5]), (rew.cpu(), z, z),
                (torch.zeros(16, device="cuda")[::2], z, z)):
        with pytest.raises(ValueError):
            st.step(*bad)
    st.step(rew, z, z.to(torch.uint8))
    assert int(st.meta[2]) == 1


def test_two_runs_give_equal_bits():
    a, _ = run_pair(2049, 100, True)
    b, _ = run_pair(2049, 100, True)
    for k in TENSORS:
        assert torch.equal(getattr(a, k), getattr(b, k))


def test_steps_replayed_from_a_graph():
    """6 step calls captured in one linear graph and replayed give the eager bits"""
    E = 1025
    _, (drew, dterm, dtrunc) = device_stream(E, 6)
    eager = EpisodeStats(E, 0, capacity=100, ring=True)
    for t in range(6):
        eager.step(drew[t], dterm[t], dtrunc[t])
    st = EpisodeStats(E, 0, capacity=100, ring=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                   # one linear chain of six launches
        for t in range(6):
            st.step(drew[t], dterm[t], dtrunc[t])
    assert int(st.meta[2]) == 0                 # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert int(eager.meta[0]) > 100 and int(eager.meta[2]) == 6
    for k in TENSORS:
        assert torch.equal(getattr(eager, k), getattr(st, k))
