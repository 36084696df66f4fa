"""The drone camera without a GPU (csrc/camera_core.h, csrc/camera_host.cpp, include/adrp.h adrp_race_camera,
gym_pybullet_adrp_amd/camera.py).

* csrc/camera_host, the CPU build of the very header the kernel compiles, against the numpy reference
  (tests/camera_reference.py) on the constructed set at 64 x 48, 17 x 9 and 1 x 1, with float64 and float32 state
  planes and with the frustum cull on and off: seg and rgb exact on decided pixels, dep and linear_depth(dep)
  within 4 x the largest float32-to-float64 difference of the reference itself on the same poses (every ray of
  the three sizes together; floors 2^-22), computed here at run time.  Before anything is compared the reference
  alone must find the set what it claims to be: at most 8 % of an image's pixels undecided, at least 10 % of all
  pixels on a gate, an obstacle or a drone, every (kind, link) pair, the ground and the sky the decided answer of
  at least 20 pixels.
* the reference's own invariants: the depth round trip, the ray through the image centre, a box filling the
  view, a drone at a known offset.
* the ctypes mirror of adrp_race_camera_io and every refusal of adrp_race_camera / adrp_race_camera_env, reached
  without a device; the refusals of adrp_race_camera_env that need a handle (persistent mode, a non-race handle,
  another E or N) and MultiRaceAviary's obs=RGB are in test_camera_gpu.py.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import camera_reference as C
from gym_pybullet_adrp_amd import _lib, camera
from gym_pybullet_adrp_amd.utils import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000      # never dereferenced by a refusal


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- the set, by the reference alone ----------------------------------------------------------------------------

@pytest.mark.parametrize("W, H", C.SIZES)
def test_constructed_set_is_what_it_claims(W, H):
    refs = C.check_set(W, H, coverage=(W, H) == (64, 48))
    assert len(refs) == 24
    dep_bar, z_bar, ddep, dz = C.bars()
    print(f"{W}x{H}: undecided max {max(1 - r['decided'].mean() for r in refs):.3f}; reference float32 vs float64: "
          f"dep {ddep:.3g}, linear depth {dz:.3g} relative")
    assert dep_bar >= 2.0 ** -22 and z_bar >= 2.0 ** -22


# ---- camera_host against the reference ----------------------------------------------------------------------------

@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("W, H", C.SIZES[:2])
def test_camera_host_equals_reference(tmp_path, W, H, dtype, cull):
    refs = C.check_set(W, H, coverage=(W, H) == (64, 48))
    dep_bar, z_bar, _, _ = C.bars()
    dep, seg, rgb = C.run_camera_host(C.constructed_envs(), W, H, tmp_path, dtype, cull)
    C.compare(refs, dep, seg, rgb, dep_bar, z_bar, f"camera_host {W}x{H}")
    for k, r in enumerate(refs):       # nothing hit: exactly 1, -1, 0 0 0 0
        sky = r["decided"] & (r["seg"] == -1)
        assert (dep[k][sky] == 1.0).all() and (seg[k][sky] == -1).all() and (rgb[k][sky] == 0).all()


def test_cull_changes_no_pixel(tmp_path):
    """the frustum cull drops only primitives no ray can reach: every pixel, decided or not, keeps its bits"""
    a = C.run_camera_host(C.constructed_envs(), 64, 48, tmp_path, np.float32, 1)
    b = C.run_camera_host(C.constructed_envs(), 64, 48, tmp_path, np.float32, 0)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_camera_host_refuses_bad_files(tmp_path):
    exe = C.build_camera_host()
    bad = tmp_path / "bad.bin"
    np.zeros(7, np.int32).tofile(bad)
    r = subprocess.run([exe, str(bad), str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert r.returncode == 2 and "header" in r.stderr
    hd = np.zeros(16, np.int32)
    hd[:6] = 1, 2, 4, 4, 4, 4
    with open(bad, "wb") as f:
        f.write(hd.tobytes() + bytes(100))
    r = subprocess.run([exe, str(bad), str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert r.returncode == 2 and "state planes" in r.stderr
    assert subprocess.run([exe], capture_output=True).returncode == 2


# ---- the reference's own invariants ---------------------------------------------------------------------------------

def test_depth_round_trip():
    z = np.geomspace(C.NEAR, C.FAR, 200)
    dep = C.depth_buffer(z)
    assert dep[0] == 0.0 and abs(dep[-1] - 1.0) < 1e-15 and (np.diff(dep) > 0).all()
    np.testing.assert_allclose(camera.linear_depth(dep), z, rtol=1e-9)
    assert camera.linear_depth(1.0) == pytest.approx(C.FAR) and camera.linear_depth(0.0) == pytest.approx(C.NEAR)
    assert (camera.NEAR, camera.FAR) == (C.L, 1000.0)


def _env(pos, quat, gates=None, obst=None):
    far = np.array([[90.0 + k, 90, 1, 0] for k in range(4)])
    pos, quat = np.asarray(pos, float), np.asarray(quat, float)
    return C.Env(pos, quat, far if gates is None else gates, far[:, :3] + [0, 9, 0] if obst is None else obst)


def test_centre_ray_is_forward():
    """an odd image's centre pixel has x = y = 0: its ray is f, and f is the body x axis but for the arm's 4e-5"""
    rng = np.random.default_rng(3)
    for _ in range(20):
        q = C.quat_from_rpy(*rng.uniform(-0.6, 0.6, 2), rng.uniform(-3, 3))
        pos = rng.uniform(-2, 2, 3) + [0, 0, 3]
        env = _env([pos, pos + [50, 50, 0]], [q, q])       # (holds the float32-rounded pose)
        eye, f, s, u = C.view(env.pos[0], env.quat[0])
        R = C.RS.rot_from_quat(env.quat[0])
        assert np.allclose(eye, env.pos[0] + [0, 0, C.L]) and np.linalg.norm(f - R[:, 0]) < 1e-4
        assert abs(s[2]) < 1e-12 and abs(f @ s) < 1e-12 and abs(f @ u) < 1e-12 and u[2] > 0      # no roll: up is world z
        # the ground straight ahead, pitched down: t = eye height / -f_z
        ts, _ = C.cast(env, 0, 3, 3)
        if f[2] < -0.05:
            assert abs(ts[0][4] - eye[2] / -f[2]) < 1e-12


def test_box_filling_the_view_gives_the_plane_depth():
    """a low gate's support box 0.3 m ahead of a level camera fills no view, so the obstacle's box is put across
    the whole image by standing close: every pixel's eye-space depth is the distance of its front face"""
    pos = np.array([[0.0, 0.0, 1.0], [40.0, 40.0, 1.0]])
    q = C.quat_from_rpy(0, 0, 0)
    dist = 0.06                                              # eye to the face; half the face is 0.075 > dist tan 30
    obst = np.array([[90.0, 90, 1]] * 4)
    obst[0] = [dist + 0.075, 0.0, 1.0 + C.L + 0.4]           # the box hangs 0.4 under the obstacle's origin
    r = C.reference(_env(pos, [q, q], obst=obst), 0, 9, 9)
    eye, f, _, _ = C.view(pos[0], q)
    z_face = (dist - eye[0]) / f[0] * 1.0                    # along f (not exactly x: the arm tilts it by 4e-5)
    assert (r["seg"] == C.seg_value(1 + C.N + 4 + 0, 0)).all() and (r["rgb"] == C.BROWN).all()
    assert np.abs(r["z"] - z_face).max() < 1e-5 and np.abs(r["z"] - dist).max() < 1e-5
    np.testing.assert_allclose(r["dep"], C.FAR / (C.FAR - C.NEAR) * (1 - C.NEAR / r["z"]), rtol=1e-15)
    # one step closer than the near plane: the face is entered before it, and the box is not seen
    obst[0, 0] = C.L * 0.9 + 0.075
    r = C.reference(_env(pos, [q, q], obst=obst), 0, 9, 9)
    assert (r["seg"] != C.seg_value(1 + C.N + 4 + 0, 0)).all()


def test_drone_at_a_known_offset_appears_at_the_predicted_pixel():
    rng = np.random.default_rng(5)
    W, H = 64, 48
    for _ in range(10):
        q = C.quat_from_rpy(*rng.uniform(-0.3, 0.3, 2), rng.uniform(-3, 3))
        pos = np.array([0.3, -0.2, 2.0])
        eye, f, s, u = C.view(pos, q)
        x, y, z = rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), rng.uniform(0.4, 0.8)     # x, y in NDC units
        other = eye + z * (f + x * C.TAN30 * s + y * C.TAN30 * u)
        r = C.reference(_env([pos, other], [q, C.quat_from_rpy(0, 0, 0)]), 0, W, H)
        j, i = int((x + 1) / 2 * W), int((1 - y) / 2 * H)
        assert r["seg"][i, j] == C.seg_value(1 + 1, -1) and (r["rgb"][i, j] == C.GREY).all()
        assert abs(r["z"][i, j] - z) < 0.07                  # within the cylinder's radius of its centre's depth
        ii, jj = np.nonzero(r["seg"] == C.seg_value(2, -1))
        assert abs(ii.mean() - i) <= 1.5 and abs(jj.mean() - j) <= 1.5
    # the camera's own drone is not drawn: alone over the ground it sees ground and sky only
    r = C.reference(_env([pos, pos + [30, 30, 0]], [q, q]), 0, W, H)
    assert set(np.unique(r["seg"])) <= {-1, 0}


def test_segmentation_values_and_colours():
    env = C.constructed_envs()[0]
    prims = C.primitives(env, 0)
    segs = [p[6] for p in prims]
    assert segs[:5] == [3 + ((k + 1) << 24) for k in range(5)]                 # gate 0: body 1 + N + 0, links 0..4
    assert segs[20:22] == [7, 7 + (1 << 24)] and segs[-1] == 2                 # obstacle 0: base -1, box 0; drone 1
    assert [p[7] for p in prims[:5]] == [C.GREY, C.BLUE, C.GREEN, C.RED, C.BROWN if C.GATE_LOW[0] else C.KINDABLUE]
    for c, rgb in ((.5, 128), (.9, 230), (.1, 26), (.7, 179), (.92, 235), (.87, 222), (.79, 201), (1, 255)):
        assert int(np.floor(255 * c + .5)) == rgb


# ---- the C-ABI without a device -------------------------------------------------------------------------------------

def _header_fields(name):
    text = open(os.path.join(ROOT, "include", "adrp.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)\s*(?:\[\w+\])?\s*;", body)


def test_struct_mirror_and_export(lib):
    """fourteen 32-bit fields and nine pointers on LP64; the header, the mirror and the library agree"""
    assert ctypes.sizeof(abi.AdrpRaceCameraIO) == 14 * 4 + 9 * 8
    assert _header_fields("adrp_race_camera_io") == [f[0] for f in abi.AdrpRaceCameraIO._fields_]
    assert hasattr(lib, "adrp_race_camera") and hasattr(lib, "adrp_race_camera_env")
    text = open(os.path.join(ROOT, "include", "adrp.h")).read()
    assert "#define ADRP_ABI_VERSION 2" in text           # purely additive: the ABI version stays


STATE = ("pos", "quat", "gates", "obstacles")
OUT = ("dep", "seg", "rgb")


def _io(**change):
    io = abi.AdrpRaceCameraIO()
    io.struct_size = ctypes.sizeof(abi.AdrpRaceCameraIO)
    io.num_envs, io.num_drones, io.width, io.height, io.num_gates, io.num_obstacles = 3, 2, 64, 48, 4, 4
    for k in STATE + OUT + ("step_counter", "mask"):
        setattr(io, k, PTR)
    for k, v in change.items():
        setattr(io, k, v)
    return io


SHARED_REFUSALS = [(dict(struct_size=8), "struct_size"), (dict(num_envs=0), "num_envs"), (dict(num_envs=-3), "num_envs"),
                   (dict(num_drones=0), "num_drones"), (dict(num_drones=abi.MAX_DRONES + 1), "num_drones"),
                   (dict(width=0), "width"), (dict(height=0), "height"), (dict(height=-1), "height"),
                   (dict(num_envs=2 ** 20, width=64, height=48), "2^31"), (dict(num_envs=2 ** 30, num_drones=8), "2^24"),
                   (dict(num_envs=2 ** 21, num_drones=8, width=1, height=1), "2^24"),
                   (dict(rgb=PTR + 2), "aligned"), (dict(dep=PTR + 1), "aligned"), (dict(seg=PTR + 3), "aligned"),
                   (dict(dep=None, seg=None, rgb=None), "no output"), (dict(capture_freq=-1), "capture_freq")]
HANDLELESS_REFUSALS = [(dict(num_gates=5), "num_gates"), (dict(num_gates=-1), "num_gates"),
                       (dict(num_obstacles=5), "num_obstacles"), (dict(num_obstacles=-1), "num_obstacles"),
                       (dict(precision=2), "precision"), (dict(capture_freq=20, step_counter=None), "step_counter")] + \
                      [({k: None}, "NULL state pointer") for k in STATE]


@pytest.mark.parametrize("change, word", SHARED_REFUSALS + HANDLELESS_REFUSALS)
def test_refusals(lib, change, word):
    """checked before any device call: they answer on a machine without a GPU"""
    assert lib.adrp_race_camera(ctypes.byref(_io(**change)), None) == abi.ERR_INVALID
    msg = lib.adrp_last_error(None).decode()
    assert msg.startswith("adrp_race_camera:") and word in msg


@pytest.mark.parametrize("change, word", SHARED_REFUSALS)
def test_env_refusals(lib, change, word):
    """the io is judged before the handle, so these too answer without one"""
    assert lib.adrp_race_camera_env(ctypes.byref(_io(**change)), None, None) == abi.ERR_INVALID
    msg = lib.adrp_last_error(None).decode()
    assert msg.startswith("adrp_race_camera_env:") and word in msg


def test_null_io_and_null_handle_refused(lib):
    assert lib.adrp_race_camera(None, None) == abi.ERR_INVALID
    assert lib.adrp_last_error(None).decode() == "adrp_race_camera: io is NULL"
    assert lib.adrp_race_camera_env(None, None, None) == abi.ERR_INVALID
    assert lib.adrp_last_error(None).decode() == "adrp_race_camera_env: io is NULL"
    assert lib.adrp_race_camera_env(ctypes.byref(_io()), None, None) == abi.ERR_INVALID
    assert lib.adrp_last_error(None).decode() == "adrp_race_camera_env: handle is NULL"


def test_single_outputs_are_accepted_up_to_the_state_check(lib):
    """one output pointer is enough: the refusal that follows is the next check's, not "no output" """
    for keep in OUT:
        io = _io(**{k: None for k in OUT if k != keep}, pos=None)
        assert lib.adrp_race_camera(ctypes.byref(io), None) == abi.ERR_INVALID
        assert "NULL state pointer" in lib.adrp_last_error(None).decode()


# ---- the Python surface ----------------------------------------------------------------------------------------------

def test_drone_camera_checks_its_arguments():
    class NotAnEnv:
        pass
    with pytest.raises(ValueError, match="MultiRaceAviary"):
        camera.DroneCamera(NotAnEnv())
    with pytest.raises(ValueError, match="outputs"):
        camera.DroneCamera(NotAnEnv(), outputs=("rgb", "normals"))
    with pytest.raises(ValueError, match="outputs"):
        camera.DroneCamera(NotAnEnv(), outputs=())
    with pytest.raises(ValueError, match="capture"):
        camera.DroneCamera(NotAnEnv(), capture="sometimes")
    with pytest.raises(ValueError, match="width"):
        camera.DroneCamera(NotAnEnv(), width=0)


def test_hover_envs_keep_their_refusal():
    from gym_pybullet_adrp_amd.envs.hover import HoverAviary
    from gym_pybullet_adrp_amd.envs.multihover import MultiHoverAviary
    from gym_pybullet_adrp_amd.utils.enums import ObservationType
    for cls in (HoverAviary, MultiHoverAviary):
        with pytest.raises(ValueError):
            cls(obs=ObservationType.RGB)
