"""CPU side of the camera-defined ray sets (esr_nerf_amd/camera.py): the float64 restatement of tests/camera_ref.py against
the reference-generated record (tests/golden/camera_rays.npz, tools/gen_camera_rays_golden.py), the binary32 colour recipe over
every (colour, alpha) pair, the constructors' float32 rounding, the refusals, the C ABI's declarations, and the condition on
the cameras of the GPU filter test."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import camera_ref as CR
import ray_filter_ref as R
from conftest import load_npz
from esr_nerf_amd import _lib, camera
from esr_nerf_amd.camera import Cameras

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("esr_camera_rays", "esr_camera_batch", "esr_camera_bounds", "esr_ray_filter_cameras")


def _golden():
    z = load_npz("camera_rays.npz")
    return z, int(z["width"]), int(z["height"])


def test_restatement_agrees_with_the_reference_record():
    z, W, H = _golden()
    assert (W, H) == (13, 7) and len(z["transform_matrices"]) == 3
    poses = CR.blender_poses(z["transform_matrices"])
    ref = CR.rays64(poses, *CR.blender_intrinsics(z["camera_angle_x"], W, H), W, H)
    rd, rv = CR.check_rays(z["rays_o"], z["rays_d"], z["viewdirs"], ref)          # origins exact, K_D and K_V hold
    print(f"golden vs float64: rays_d {rd:.3f} (K_D {CR.K_D}), viewdirs {rv:.3f} (K_V {CR.K_V})")
    # the constants are twice the reference's own worst ratio, rounded up (camera_ref.MEASURED)
    assert CR.K_D == int(np.ceil(2 * max(CR.MEASURED["rays_d"].values())))
    assert CR.K_V == int(np.ceil(2 * max(CR.MEASURED["viewdirs"].values())))
    assert rd <= CR.MEASURED["rays_d"]["golden"] + 0.01 and rv <= CR.MEASURED["viewdirs"]["golden"] + 0.01
    # one axis-aligned pose (a rotation of 0 / +-1 entries), two oblique
    rot = np.abs(poses[:, :, :3])
    assert [bool(np.isin(r, (0.0, 1.0)).all()) for r in rot] == [True, False, False]
    # the training loader gives every ray of a view its view's mode
    modes = z["em_modes"].reshape(3, W * H)
    assert z["em_modes"].dtype == np.int64 and (modes == modes[:, :1]).all() and modes[:, 0].tolist() == [0, 1, 0]


def test_bound_constants_are_twice_the_references_measured_ratios():
    """K_D and K_V follow from what ``camera_ref.measure()`` finds today (the record and 4096 seeded random poses through the
    loader's own torch expressions), not from figures written down once"""
    m = CR.measure(os.path.join(ROOT, "tests", "golden", "camera_rays.npz"))
    for i, key in enumerate(("rays_d", "viewdirs")):
        for src in ("golden", "random"):
            assert abs(m[src][i] - CR.MEASURED[key][src]) <= 0.01, (key, src, m[src][i])
    assert CR.K_D == int(np.ceil(2 * max(v[0] for v in m.values()))) == 7
    assert CR.K_V == int(np.ceil(2 * max(v[1] for v in m.values()))) == 5


def test_uint8_table_and_colour_recipe_are_the_reference_line_for_every_pair():
    table = camera.uint8_table()
    assert table.dtype == np.float32 and np.array_equal(table, np.float32(np.arange(256) / 255.0))
    assert np.array_equal(table, CR.uint8_table())
    assert np.array_equal(table, torch.FloatTensor(np.arange(256, dtype=np.uint8) / 255.0).numpy())       # esrnerf.py:159-161
    c, a = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    cf, af = torch.from_numpy(table[c]), torch.from_numpy(table[a])
    for white_bg in (True, False, 1.0, 0.0):
        want = cf * af + (1 - af) * white_bg                                                # esrnerf.py:236, in torch float32
        got = CR.composite32(c, a, white_bg)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32)), white_bg
    z, _, _ = _golden()
    alpha = z["rgba"][:, 3]
    assert (alpha == 0).any() and (alpha == 255).any() and ((alpha > 0) & (alpha < 255)).any()
    for tag, white_bg in (("white", True), ("black", False)):
        got = CR.composite_rgba(z["rgba"], white_bg)
        assert np.array_equal(got.view(np.uint32), z[f"rgbs_{tag}"].view(np.uint32)), tag


def test_constructors_round_to_float32_where_the_loaders_do():
    z, W, H = _golden()
    cams = Cameras.from_blender(z["transform_matrices"], float(z["camera_angle_x"]), W, H)
    fx, fy, cx, cy = CR.blender_intrinsics(z["camera_angle_x"], W, H)
    assert (cams.fx, cams.fy, cams.cx, cams.cy) == (fx, fy, cx, cy)
    assert cams.fx == float(np.float32(float(z["focal"]))) and cams.fx != float(z["focal"])      # rounded, not the float64
    assert (cams.width, cams.height, cams.n_views, cams.n_rays) == (W, H, 3, 3 * W * H)
    assert cams.poses.dtype == torch.float32 and np.array_equal(cams.poses.numpy(), CR.blender_poses(z["transform_matrices"]))
    # the loader's float32 poses, with the y and z columns flipped (pose @ blender2opencv)
    assert np.array_equal(cams.poses.numpy(), z["poses_f32"][:, :3, :] * np.float32([1, -1, -1, 1]))
    assert np.array_equal(cams.poses[:, :, 3].numpy(), z["rays_o"].reshape(3, W * H, 3)[:, 0])
    poses, K, w, h = CR.intrinsics_set()
    ci = Cameras.from_intrinsics(poses, K, w, h)
    assert (ci.fx, ci.fy, ci.cx, ci.cy) == tuple(float(np.float32(v)) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    assert ci.fx != ci.fy and ci.cx != w * 0.5 and ci.cy != h * 0.5 and ci.fx != K[0, 0]
    full = np.concatenate([poses, np.broadcast_to(np.float32([0, 0, 0, 1]), (2, 1, 4))], 1)
    assert torch.equal(Cameras.from_intrinsics(torch.from_numpy(full), np.pad(K, (0, 1)), w, h).poses, ci.poses)
    s = ci.struct()
    assert (s.fx, s.width, s.height, s.n_views) == (ci.fx, w, h, 2)


def test_misuse_is_refused_with_a_message():
    poses = torch.zeros(2, 3, 4)
    with pytest.raises(ValueError, match="2\\^31"):
        Cameras(poses, 1.0, 1.0, 0.5, 0.5, 65536, 16384)                       # 2 * 2^30 rays
    Cameras(poses, 1.0, 1.0, 0.5, 0.5, 65536, 16383)                           # one row fewer per view: accepted
    with pytest.raises(ValueError, match="float32"):
        Cameras(poses.double(), 1.0, 1.0, 0.5, 0.5, 4, 4)
    with pytest.raises(ValueError, match=r"\[V, 3, 4\]"):
        Cameras(torch.zeros(2, 4, 4), 1.0, 1.0, 0.5, 0.5, 4, 4)
    with pytest.raises(ValueError, match="non-zero"):
        Cameras(poses, 0.0, 1.0, 0.5, 0.5, 4, 4)
    for bad in (float("nan"), float("inf")):
        broken = poses.clone()
        broken[1, 2, 3] = bad
        with pytest.raises(ValueError, match="finite"):
            Cameras(broken, 1.0, 1.0, 0.5, 0.5, 4, 4)
    cams = Cameras(poses, 1.0, 1.0, 0.5, 0.5, 4, 3)
    n = cams.n_rays
    for bad in (torch.tensor([0, n]), torch.tensor([-1, 3])):
        with pytest.raises(ValueError, match="out of range"):
            camera.validate_rows(cams, bad)
    camera.validate_rows(cams, torch.tensor([0, n - 1, 5, 5]))
    camera.validate_rows(cams, torch.zeros(0, dtype=torch.int64))
    for bad in (torch.tensor([0, 1], dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64), [0, 1]):
        with pytest.raises(ValueError, match="int64 vector"):
            camera.validate_rows(cams, bad)
    images, modes = torch.zeros(n, 4, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
    assert camera.check_images(cams, images, modes) == 4 and camera.check_images(cams, torch.zeros(n, 3), modes) == 0
    for bad_img, bad_modes in ((images[:, :2], modes), (images.float(), modes), (images[:-1], modes), (images, modes.int()),
                               (images, modes[:1]), (torch.zeros(n, 3, dtype=torch.float64), modes)):
        with pytest.raises(ValueError):
            camera.check_images(cams, bad_img, bad_modes)
    rows = torch.tensor([0, 1])
    with pytest.raises(ValueError, match="int64 vector"):
        camera.camera_batch(cams, images, modes, rows.int(), 1.0)
    # CPU tensors: there is no CPU kernel
    for call in (lambda: camera.camera_rays(cams), lambda: camera.camera_batch(cams, images, modes, rows, 1.0),
                 lambda: camera.frustum_bbox(cams, 2.0, 6.0), lambda: camera.filter_camera_rays(None, cams, True)):
        with pytest.raises(RuntimeError, match="needs device tensors"):
            call()
    from esr_nerf_amd.evaluate import render_camera_view
    with pytest.raises(RuntimeError, match="needs device tensors"):
        render_camera_view(None, cams, 0, 0, None, 16)
    with pytest.raises(ValueError, match="provides"):
        camera._check_keys(["rays_o", "hdrs"])


def test_header_declares_the_camera_entry_points_and_ctypes_agrees():
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    # the names only: tests/test_host.py checks every entry's restype and argument types against the header text
    for name in ENTRIES:
        assert name in _lib.EXPORTS and _lib.SIGNATURES[name][0] is ctypes.c_int, name
    assert int(re.search(r"#define ESR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    for name, val in (("ESR_CAMERA_LDS_VIEWS", _lib.CAMERA_LDS_VIEWS), ("ESR_CAMERA_BOUNDS_BLOCKS", _lib.CAMERA_BOUNDS_BLOCKS)):
        assert int(re.search(r"#define " + name + r" (\d+)", header).group(1)) == val
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "esr_hip.h"\nint main(){printf("%zu %zu %zu",'
           'sizeof(esr_camera_t),offsetof(esr_camera_t,width),offsetof(esr_camera_t,n_views));return 0;}')
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes == [ctypes.sizeof(_lib.EsrCamera), _lib.EsrCamera.width.offset, _lib.EsrCamera.n_views.offset]


def test_entry_points_refuse_a_bad_camera_before_any_launch():
    """The argument checks of the C entries run on the host, so they can be exercised without a GPU: a zero focal length, an
    empty image and 2^31 rays are ESR_EINVAL from every entry, the filter's included"""
    L = _lib.lib()
    scene = _lib.EsrScene()
    null = ctypes.c_void_p(0)
    for cam in (_lib.EsrCamera(0.0, 1.0, 0.5, 0.5, 4, 4, 1), _lib.EsrCamera(1.0, 0.0, 0.5, 0.5, 4, 4, 1),
                _lib.EsrCamera(1.0, 1.0, 0.5, 0.5, 0, 4, 1), _lib.EsrCamera(1.0, 1.0, 0.5, 0.5, 65536, 16384, 2)):
        c = ctypes.byref(cam)
        assert L.esr_ray_filter_cameras(ctypes.byref(scene), null, c, null, 0, 6.0, 4, null, null, null) == -1
        assert L.esr_camera_rays(c, null, 0, 1, null, null, null, null) == -1
        assert L.esr_camera_batch(c, null, null, null, 4, null, 1.0, null, 1, null, null, null, null, null, null) == -1
        assert L.esr_camera_bounds(c, null, 2.0, 6.0, null, null, null) == -1


def test_filter_cameras_keep_a_share_strictly_between_0_and_1():
    """A condition on the INPUTS of tests/test_gpu_camera.py's filter test, checked without a GPU: the float64 classifier for
    both samplers, the renderer's retained torch loop for the fixed one (the march sampler is a library call)"""
    poses, K, w, h = CR.filter_set()
    cams = Cameras.from_intrinsics(poses, K, w, h)
    ref = CR.rays64(cams.poses.numpy(), cams.fx, cams.fy, cams.cx, cams.cy, w, h)
    ro, rd = ref["o"].astype(np.float32), ref["d"].astype(np.float32)
    _, fine = R.renderers("cpu")
    S = R.scene_of(fine)
    for fixed in (True, False):
        c = R.classify(S, ro, rd, fixed)
        kept = float((c["cls"] == R.KEEP).mean())
        dropped = float((c["cls"] == R.DROP).mean())
        assert kept > 0.1 and dropped > 0.1, (fixed, kept, dropped)
    fine.sdf_random_init = True
    keep = fine._filter_rays_torch(torch.from_numpy(ro), torch.from_numpy(rd), 512)
    assert 0.1 < float(keep.float().mean()) < 0.9
