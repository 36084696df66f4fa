"""The drone camera kernel on the GPU (csrc/camera_kernel.h; include/adrp.h adrp_race_camera, adrp_race_camera_env;
camera.DroneCamera; MultiRaceAviary(obs=ObservationType.RGB)).

The kernel renders the constructed set of tests/camera_reference.py (24 images: E = 3, N = 2 per launch, a
different scene per (env, drone)) at 64 x 48, 17 x 9 (under one block of pixels, a multiple of nothing) and 1 x 1,
from float64 and float32 state planes.  On decided pixels seg and rgb are exact; dep and linear_depth(dep) stay
within 4 x the largest float32-to-float64 difference of the reference itself on the same poses (every ray of the
three sizes together; floors 2^-22), computed on the CPU at run time (camera_reference.bars; tests/test_camera.py
holds the CPU twin to the same bars).  Every buffer is followed by guard words and pre-filled with a sentinel.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import camera_reference as C  # noqa: E402
from gym_pybullet_adrp_amd import _lib  # noqa: E402
from gym_pybullet_adrp_amd.camera import DroneCamera  # noqa: E402
from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary  # noqa: E402
from gym_pybullet_adrp_amd.utils import abi  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import ObservationType  # noqa: E402

E, N = 3, C.N
OUT = ("dep", "seg", "rgb")
SENTINEL, GUARD = 0x5A5A5A5A, 64
DEV = "cuda:0"


class Images:
    """dep / seg / rgb buffers of [E, N, H, W] pixels, each one int32 word per pixel plus GUARD words, all SENTINEL"""

    def __init__(self, W, H, envs=E):
        self.shape = (envs, N, H, W)
        self.px = envs * N * H * W
        self.raw = {k: torch.full((self.px + GUARD,), SENTINEL, dtype=torch.int32, device=DEV) for k in OUT}

    def ptr(self, k):
        return self.raw[k].data_ptr()

    def get(self, k):
        w = self.raw[k][:self.px].cpu().numpy()
        return {"dep": lambda: w.view(np.float32).reshape(self.shape), "seg": lambda: w.reshape(self.shape),
                "rgb": lambda: w.view(np.uint8).reshape(self.shape + (4,))}[k]()

    def words(self, k):
        return self.raw[k][:self.px].cpu().numpy().reshape(self.shape)

    def guards_intact(self):
        return all(bool((self.raw[k][self.px:] == SENTINEL).all()) for k in OUT)


def launch(planes, W, H, img, outputs=OUT, precision=1, step_counter=None, capture_freq=0, mask=None, envs=E):
    """adrp_race_camera on device planes (pos, quat, gates, obstacles) into img"""
    io = abi.AdrpRaceCameraIO()
    io.struct_size = ctypes.sizeof(abi.AdrpRaceCameraIO)
    io.num_envs, io.num_drones, io.width, io.height, io.num_gates, io.num_obstacles = envs, N, W, H, 4, 4
    for g in range(4):
        io.gate_low[g] = C.GATE_LOW[g]
    io.precision, io.capture_freq = precision, capture_freq
    io.pos, io.quat, io.gates, io.obstacles = (p.data_ptr() for p in planes)
    keep = []
    if step_counter is not None:
        keep.append(torch.as_tensor(np.repeat(step_counter, N), dtype=torch.int32, device=DEV))
        io.step_counter = keep[-1].data_ptr()
    if mask is not None:
        keep.append(torch.as_tensor(mask, dtype=torch.uint8, device=DEV))
        io.mask = keep[-1].data_ptr()
    for k in outputs:
        setattr(io, k, img.ptr(k))
    lib = _lib.load()
    rc = lib.adrp_race_camera(ctypes.byref(io), _lib._raw_stream(0))
    assert rc == 0, lib.adrp_last_error(None).decode()
    torch.cuda.synchronize()


def device_planes(envs, precision):
    dt = np.float64 if precision else np.float32
    return [torch.from_numpy(a).to(DEV) for a in C.planes(envs, dt)]


def render_set(W, H, precision):
    """the 24 images of the constructed set, three envs per launch: dep, seg, rgb [24, H, W(, 4)]"""
    envs = C.constructed_envs()
    out = {k: [] for k in OUT}
    for at in range(0, len(envs), E):
        img = Images(W, H)
        launch(device_planes(envs[at:at + E], precision), W, H, img, precision=precision)
        assert img.guards_intact()
        for k in OUT:
            a = img.get(k)
            out[k].append(a.reshape((E * N,) + a.shape[2:]))
    return [np.concatenate(out[k]) for k in OUT]


@pytest.mark.parametrize("precision", [1, 0], ids=["fp64", "fp32"])
@pytest.mark.parametrize("W, H", C.SIZES)
def test_kernel_equals_reference(W, H, precision):
    refs = C.check_set(W, H, coverage=(W, H) == (64, 48))       # the set's conditions, on the CPU, first
    dep_bar, z_bar, _, _ = C.bars()
    dep, seg, rgb = render_set(W, H, precision)
    C.compare(refs, dep, seg, rgb, dep_bar, z_bar, f"kernel {W}x{H} {'fp64' if precision else 'fp32'} planes")
    for k, r in enumerate(refs):       # nothing hit: exactly 1, -1, 0 0 0 0
        sky = r["decided"] & (r["seg"] == -1)
        assert (dep[k][sky] == 1.0).all() and (rgb[k][sky] == 0).all()


def test_fp32_and_fp64_planes_give_the_same_seg():
    W, H = 64, 48
    refs = C.check_set(W, H)
    _, s64, c64 = render_set(W, H, 1)
    _, s32, c32 = render_set(W, H, 0)
    for k, r in enumerate(refs):
        m = r["decided"]
        assert (s64[k][m] == s32[k][m]).all() and (c64[k][m] == c32[k][m]).all()


def test_single_outputs_null_outputs_and_repeat_launches():
    """each output alone equals the same output rendered with the others; an output not asked for is not written;
    two launches give identical bits"""
    W, H = 17, 9
    planes = device_planes(C.constructed_envs()[:E], 1)
    full, again = Images(W, H), Images(W, H)
    launch(planes, W, H, full)
    launch(planes, W, H, again)
    for k in OUT:
        assert np.array_equal(full.words(k), again.words(k))
        assert not (full.words(k) == SENTINEL).any()
        alone = Images(W, H)
        launch(planes, W, H, alone, outputs=(k,))
        assert np.array_equal(alone.words(k), full.words(k)) and alone.guards_intact()
        for other in OUT:
            if other != k:
                assert (alone.words(other) == SENTINEL).all()
    assert full.guards_intact() and again.guards_intact()


def test_capture_schedule_and_mask():
    W, H = 17, 9
    planes = device_planes(C.constructed_envs()[3:3 + E], 0)
    full = Images(W, H)
    launch(planes, W, H, full, precision=0)
    sched = Images(W, H)
    launch(planes, W, H, sched, precision=0, step_counter=[0, 20, 40], capture_freq=40)
    masked = Images(W, H)
    launch(planes, W, H, masked, precision=0, mask=[0, 1, 0])
    both = Images(W, H)       # schedule and mask together: env 2 alone (on schedule and unmasked)
    launch(planes, W, H, both, precision=0, step_counter=[0, 20, 40], capture_freq=40, mask=[0, 1, 1])
    always = Images(W, H)     # capture_freq 0 renders whatever the counters say
    launch(planes, W, H, always, precision=0, step_counter=[7, 13, 1], capture_freq=0)
    for k in OUT:
        for img, rendered in ((sched, (0, 2)), (masked, (1,)), (both, (2,)), (always, (0, 1, 2))):
            for e in range(E):
                if e in rendered:
                    assert np.array_equal(img.words(k)[e], full.words(k)[e])
                else:
                    assert (img.words(k)[e] == SENTINEL).all()
            assert img.guards_intact()


def _state_planes(env):
    f, i = env.get_state()
    names = env.state_field_names()[0]
    rows = lambda first, count: f[names.index(first):names.index(first) + count].contiguous()      # noqa: E731
    return rows("pos_x", 3), rows("quat_x", 4), rows("gate_0_x", 16), rows("obst_0_x", 12), i[0].contiguous()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_env_call_equals_handleless_call(precision):
    """level2 moves every env's gates and obstacles by its own offsets: an env-indexing error shows"""
    env = MultiRaceAviary("level2", num_drones=N, num_envs=E, seed=5, precision=precision)
    try:
        obs, _ = env.reset()
        act = torch.cat([obs[..., :3] + torch.tensor([0.1, 0.0, 0.6], device=obs.device), torch.zeros_like(obs[..., :1])], -1)
        for _ in range(4):
            env.step(act.contiguous())
        cam = DroneCamera(env, 64, 48)
        got = {k: v.clone() for k, v in cam.render().items()}
        pos, quat, gates, obst, _ = _state_planes(env)
        assert float((gates[0].reshape(E, N)[1:, 0] - gates[0, 0]).abs().min()) > 0      # the envs' gates do differ
        want = cam.render_poses(pos, quat, gates, obst)
        torch.cuda.synchronize()
        for k in OUT:
            assert torch.equal(got[k], want[k]), k
        assert cam.render()["rgb"] is cam.rgb and cam.dep is cam.images["dep"]           # the same tensors every call
        assert int((got["seg"] > 0).sum()) > 0                                            # something besides ground and sky
    finally:
        env.close()


def test_race_env_rgb_observation():
    kw = dict(num_drones=N, num_envs=2, seed=11, autoreset=True)
    env = MultiRaceAviary("level2", obs=ObservationType.RGB, **kw)
    kin = MultiRaceAviary("level2", obs=ObservationType.KIN, **kw)
    try:
        sp = env.observation_space
        assert sp.shape == (N, 48, 64, 4) and sp.dtype == np.uint8 and sp.low.min() == 0 and sp.high.max() == 255
        assert kin.observation_space.shape == (N, 49) and kin.camera is None

        def check(obs):
            assert obs.shape == (2, N, 48, 64, 4) and obs.dtype == torch.uint8 and obs.is_cuda
            pos, quat, gates, obst, _ = _state_planes(env)
            want = env.camera.render_poses(pos, quat, gates, obst)
            for k in OUT:
                assert torch.equal(env.camera.images[k], want[k]), k
            assert torch.equal(obs, want["rgb"])

        obs, info = env.reset()
        kobs, _ = kin.reset()
        check(obs)
        assert torch.equal(env.kin_obs, kobs)
        assert env.camera.dep.dtype == torch.float32 and env.camera.seg.dtype == torch.int32
        act = torch.cat([kobs[..., :3] + torch.tensor([0.0, 0.1, 0.5], device=kobs.device), torch.zeros_like(kobs[..., :1])], -1)
        act = act.contiguous()
        for _ in range(5):
            obs, rew, term, trunc, info = env.step(act)
            kobs, krew, kterm, ktrunc, _ = kin.step(act)
            check(obs)
            assert torch.equal(env.kin_obs, kobs) and torch.equal(rew, krew)
            assert torch.equal(term, kterm) and torch.equal(trunc, ktrunc)
        assert obs.data_ptr() == env.camera.rgb.data_ptr()

        # env 0 flies out of bounds: the step ends its episode and resets it; its images show the start pose
        f, i = env.get_state()
        names, inames = env.state_field_names()
        f[names.index("pos_z"), :N] = 50.0
        env.set_state(f, i)
        start = torch.tensor(np.array(env.cfg.track.init_pos)[:N], device=f.device)
        obs, rew, term, trunc, info = env.step(act)
        assert bool(term[0]) and not bool(term[1])
        f, i = env.get_state()
        assert (i[inames.index("step_counter"), :N] == 0).all() and (i[inames.index("step_counter"), N:] > 0).all()
        p = torch.stack([f[names.index(n), :N] for n in ("pos_x", "pos_y", "pos_z")], -1).double()
        assert float((p - start).abs().max()) <= 0.1 + 1e-6            # level2 draws the start within +-0.1 (z: 0.02)
        check(obs)
    finally:
        env.close()
        kin.close()


def _env_io(envs, drones, img):
    io = abi.AdrpRaceCameraIO()
    io.struct_size = ctypes.sizeof(abi.AdrpRaceCameraIO)
    io.num_envs, io.num_drones, io.width, io.height = envs, drones, 17, 9
    for k in OUT:
        setattr(io, k, img.ptr(k))
    return io


def _refused(io, handle, word):
    lib = _lib.load()
    assert lib.adrp_race_camera_env(ctypes.byref(io), handle, _lib._raw_stream(0)) == abi.ERR_INVALID
    msg = lib.adrp_last_error(None).decode()
    assert msg.startswith("adrp_race_camera_env:") and word in msg, msg


def test_env_call_refuses_the_wrong_handle():
    """the refusals of adrp_race_camera_env that need a handle: a hover handle, a hover handle in persistent mode,
    a race handle of another E or N; nothing is launched, so nothing is written"""
    from gym_pybullet_adrp_amd.envs.hover import HoverAviary
    img = Images(17, 9)
    hover = HoverAviary(num_envs=E)
    race = MultiRaceAviary("level0", num_drones=N, num_envs=2)
    try:
        hover.reset()
        _refused(_env_io(E, 1, img), hover.h.h, "not a MultiRaceAviary handle")
        with hover.persistent() as p:
            p.step(np.zeros((E, 1, hover.h.A), np.float32))
            _refused(_env_io(E, 1, img), hover.h.h, "persistent mode")
        race.reset()
        _refused(_env_io(E, N, img), race.h.h, "differ from the handle's")          # another E
        _refused(_env_io(2, 1, img), race.h.h, "differ from the handle's")          # another N
        torch.cuda.synchronize()
        for k in OUT:
            assert (img.raw[k] == SENTINEL).all()
        lib = _lib.load()                                                           # the right shape is taken
        assert lib.adrp_race_camera_env(ctypes.byref(_env_io(2, N, Images(17, 9, envs=2))), race.h.h, _lib._raw_stream(0)) == 0
        torch.cuda.synchronize()
    finally:
        hover.close()
        race.close()
