"""Camera-defined ray sets on the MI355X (esr_nerf_amd/camera.py over csrc/camera.hip and the camera instantiation of
csrc/rayfilter.hip): dense rays against the float64 restatement of tests/camera_ref.py, batches against the dense rays and
the reference-generated record (tests/golden/camera_rays.npz), the colour recipe over every (colour, alpha) pair, both
pose-table paths of the batch kernel, the camera samplers against the array samplers, the filter, the frustum bounds and
``render_camera_view``."""
import numpy as np
import pytest
import torch

import camera_ref as CR
import ray_filter_ref as R
from conftest import load_npz
from esr_nerf_amd import _lib
from esr_nerf_amd.config import AttrDict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ["rgbs", "rays_o", "rays_d", "viewdirs", "em_modes"]
U = 2.0 ** -24


def _bits(a, b):
    """bit-for-bit equality of two tensors (NaN-safe, -0 != +0)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {torch.float32: torch.int32, torch.float64: torch.int64}.get(a.dtype)
    return torch.equal(a.view(view), b.view(view)) if view else torch.equal(a, b)


@pytest.fixture(scope="module")
def gold():
    from esr_nerf_amd.camera import Cameras
    z = load_npz("camera_rays.npz")
    W, H = int(z["width"]), int(z["height"])
    cams = Cameras.from_blender(z["transform_matrices"], float(z["camera_angle_x"]), W, H, device=DEV)
    modes = torch.from_numpy(z["em_modes"].reshape(3, -1)[:, 0].copy()).to(DEV)
    return dict(z=z, cams=cams, rgba=torch.from_numpy(z["rgba"]).to(DEV), modes=modes)


@pytest.fixture(scope="module")
def small():
    from esr_nerf_amd.camera import Cameras
    poses, K, w, h = CR.intrinsics_set()
    return Cameras.from_intrinsics(poses, K, w, h, device=DEV)


def _ref_of(cams):
    return CR.rays64(cams.poses.cpu().numpy(), cams.fx, cams.fy, cams.cx, cams.cy, cams.width, cams.height)


def test_dense_rays_against_float64(gold, small):
    from esr_nerf_amd.camera import camera_rays
    for name, cams in (("golden 3 x 13x7", gold["cams"]), ("intrinsics 2 x 5x3", small)):
        ro, rd, vd = camera_rays(cams)
        assert ro.shape == rd.shape == vd.shape == (cams.n_rays, 3) and ro.dtype == torch.float32
        worst_d, worst_v = CR.check_rays(ro.cpu().numpy(), rd.cpu().numpy(), vd.cpu().numpy(), _ref_of(cams))
        print(f"{name}: worst rays_d ratio {worst_d:.3f} (K_D {CR.K_D}), viewdirs {worst_v:.3f} (K_V {CR.K_V})")
        hw = cams.width * cams.height
        for views, sl in ((1, slice(hw, 2 * hw)), ((1, cams.n_views), slice(hw, None)), (range(0, 1), slice(0, hw)),
                          ((1, 1), slice(0, 0))):
            part = camera_rays(cams, views)
            assert all(_bits(p, w[sl]) for p, w in zip(part, (ro, rd, vd))), (name, views)
    # the record itself: the loader's own float32 rays lie within the same bounds of the kernel's (twice, by the triangle)
    z = gold["z"]
    ro, rd, vd = (t.cpu().numpy() for t in camera_rays(gold["cams"]))
    assert np.array_equal(ro, z["rays_o"])
    ref = _ref_of(gold["cams"])
    assert (np.abs(rd.astype(np.float64) - z["rays_d"]) <= 2 * CR.K_D * U * ref["dabs"]).all()
    assert (np.abs(vd.astype(np.float64) - z["viewdirs"]) <= 2 * CR.K_V * U).all()


def _rows(cams, n):
    """first and last pixel of every view, repeats, then every row in descending order; cut to n"""
    hw, N = cams.width * cams.height, cams.n_rays
    ends = [r for v in range(cams.n_views) for r in (v * hw, v * hw + hw - 1)]
    rows = ends + [5, 5, 5, N - 1, N - 1] + list(range(N - 1, -1, -1))
    return torch.tensor(rows[:n], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 200])
def test_batch_rows(gold, n):
    from esr_nerf_amd.camera import camera_batch, camera_rays
    cams, z = gold["cams"], gold["z"]
    rows = _rows(cams, n)
    assert len(rows) == n
    dense = camera_rays(cams)
    table = torch.from_numpy(CR.uint8_table()).to(DEV)
    for tag, white_bg in (("white", True), ("black", False)):
        b = camera_batch(cams, gold["rgba"], gold["modes"], rows, white_bg)
        assert list(b) == ["rays_o", "rays_d", "viewdirs", "rgbs", "em_modes"]
        for k, want in zip(("rays_o", "rays_d", "viewdirs"), dense):
            assert b[k].shape == (n, 3) and _bits(b[k], want[rows]), (k, n)
        assert b["em_modes"].dtype == torch.int64 and torch.equal(b["em_modes"].cpu(), torch.from_numpy(z["em_modes"])[rows.cpu()])
        assert _bits(b["rgbs"].cpu(), torch.from_numpy(z[f"rgbs_{tag}"])[rows.cpu()]), (tag, n)
    rgb8 = gold["rgba"][:, :3].contiguous()
    b = camera_batch(cams, rgb8, gold["modes"], rows, True)
    assert _bits(b["rgbs"], table[rgb8[rows].long()])
    comp = torch.from_numpy(z["rgbs_white"]).to(DEV)
    b = camera_batch(cams, comp, gold["modes"], rows, 0.0)
    assert _bits(b["rgbs"], comp[rows]) and _bits(b["rays_d"], dense[1][rows])


def test_batch_refuses_rows_out_of_range_and_mixed_devices(gold):
    from esr_nerf_amd.camera import camera_batch
    cams = gold["cams"]
    for bad in ([0, cams.n_rays], [-1]):
        with pytest.raises(ValueError, match="out of range"):
            camera_batch(cams, gold["rgba"], gold["modes"], torch.tensor(bad, device=DEV), True)
    with pytest.raises(RuntimeError, match="needs device tensors"):
        camera_batch(cams, gold["rgba"], gold["modes"], torch.tensor([0]), True)


def test_every_colour_alpha_pair_is_the_host_recipe():
    from esr_nerf_amd.camera import Cameras, camera_batch
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rgba = np.stack([c, 255 - c, c[::-1], a], -1).reshape(-1, 4)                    # one 256 x 256 view, every (c, a)
    cams = Cameras(torch.from_numpy(CR.look_at_cv((1.0, 2.0, 3.0), (0, 0, 0)))[None].to(DEV), 300.0, 300.0, 128.0, 128.0, 256, 256)
    rows = torch.arange(cams.n_rays, device=DEV)
    modes = torch.tensor([1], device=DEV)
    for white_bg in (True, False):
        b = camera_batch(cams, torch.from_numpy(rgba).to(DEV), modes, rows, white_bg)
        want = CR.composite_rgba(rgba, white_bg)
        assert np.array_equal(b["rgbs"].cpu().numpy().view(np.uint32), want.view(np.uint32)), white_bg
        assert bool((b["em_modes"] == 1).all())


def test_pose_table_in_lds_and_in_global_memory():
    """view counts at and just over ESR_CAMERA_LDS_VIEWS, 1 x 1 images: the two instantiations of the batch kernel"""
    from esr_nerf_amd.camera import Cameras, camera_batch, camera_rays
    rng = np.random.default_rng(3)
    cap = _lib.CAMERA_LDS_VIEWS
    eyes = rng.normal(size=(cap + 1, 3))
    eyes *= (3.0 / np.linalg.norm(eyes, axis=-1, keepdims=True))
    poses = torch.from_numpy(np.stack([CR.look_at_cv(e, rng.uniform(-0.3, 0.3, 3)) for e in eyes]))
    rgba = torch.from_numpy(rng.integers(0, 256, (cap + 1, 4), dtype=np.uint8))
    modes = torch.from_numpy(rng.integers(0, 5, cap + 1))
    for v in (cap, cap + 1):
        cams = Cameras(poses[:v].to(DEV), 1.3, 1.1, 0.4, 0.7, 1, 1)
        rows = torch.from_numpy(rng.permutation(np.repeat(np.arange(v), 2))).to(DEV)
        b = camera_batch(cams, rgba[:v].to(DEV), modes[:v].to(DEV), rows, True)
        dense = camera_rays(cams)
        CR.check_rays(*(t.cpu().numpy() for t in dense), _ref_of(cams))
        for k, want in zip(("rays_o", "rays_d", "viewdirs"), dense):
            assert _bits(b[k], want[rows]), (v, k)
        assert torch.equal(b["em_modes"].cpu(), modes[rows.cpu()])
        assert np.array_equal(b["rgbs"].cpu().numpy().view(np.uint32), CR.composite_rgba(rgba.numpy()[rows.cpu().numpy()], True).view(np.uint32))


def _cfg(preload="cuda"):
    return AttrDict(system=dict(device=DEV, data_preload=preload), data=dict(white_bg=True))


def _arrays(gold):
    from esr_nerf_amd.camera import camera_rays
    ro, rd, vd = camera_rays(gold["cams"])
    hw = gold["cams"].width * gold["cams"].height
    return dict(rays_o=ro, rays_d=rd, viewdirs=vd, rgbs=torch.from_numpy(CR.composite_rgba(gold["z"]["rgba"], True)).to(DEV),
                em_modes=gold["modes"].repeat_interleave(hw))


def _same(x, y):
    assert list(x) == list(y)
    for k in x:
        assert _bits(x[k], y[k]), k


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_camera_batch_sampler_returns_the_array_samplers_batches(gold, rank, world):
    from esr_nerf_amd.camera import CameraBatchSampler
    from esr_nerf_amd.data import BatchSampler
    data = _arrays(gold)
    n = gold["cams"].n_rays
    mask = (torch.arange(n, device=DEV) % 7) != 3

    def run(make):
        torch.manual_seed(11)
        s = make()
        s.shuffle()
        out = [s.sample() for _ in range(12)]              # 273 rays, batches of 32: crosses a reshuffle
        s.filter(mask[s.data_idxs])
        out += [s.sample() for _ in range(18)]             # 234 rays left: two more reshuffles
        return s, out

    a, xa = run(lambda: BatchSampler(_cfg(), data, KEYS, 32, rank=rank, world=world))
    c, xc = run(lambda: CameraBatchSampler(_cfg(), gold["cams"], gold["rgba"], gold["modes"], KEYS, 32, rank=rank, world=world))
    assert len(xa) == len(xc) == 30
    for x, y in zip(xa, xc):
        _same(x, y)
        assert len(x["rgbs"]) == 32 // world
    assert torch.equal(a.data_idxs, c.data_idxs) and (a.batch_st, a.data_num) == (c.batch_st, c.data_num) and c.data_num < n
    assert _bits(a.current("rays_d"), c.current("rays_d")) and _bits(a.current("rgbs"), c.current("rgbs"))
    # checkpointed state is interchangeable between the two forms; data_preload: cpu is accepted and the set stays on the device
    again = CameraBatchSampler(_cfg("cpu"), gold["cams"].to("cpu"), gold["rgba"].cpu(), gold["modes"].cpu(), KEYS, 32,
                               a.batch_st, a.data_idxs.cpu().clone(), rank=rank, world=world)
    assert again.data_idxs.is_cuda and again.images.is_cuda and not again.data_preload_to_cpu
    torch.manual_seed(4)
    x = [a.sample() for _ in range(9)]
    torch.manual_seed(4)
    y = [again.sample() for _ in range(9)]
    for p, q in zip(x, y):
        _same(p, q)


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_camera_ray_group_manager_returns_the_array_managers_batches(gold, rank, world):
    from esr_nerf_amd.camera import CameraRayGroupManager
    from esr_nerf_amd.data import RayGroupManager
    data = _arrays(gold)
    n = gold["cams"].n_rays

    def run(make):
        torch.manual_seed(23)
        s = make()
        s.shuffle()
        out = [s.sample() for _ in range(10)]              # no certain ray yet: the whole-mask quirk; crosses a reshuffle
        s.filter((s.uncert_data_idxs % 3) != 0)            # a third of the rays move to the certain group
        out += [s.sample() for _ in range(10)]
        s.filter((s.uncert_data_idxs % 5) != 1)            # regrouping: more rays join the END of the certain group
        out += [s.sample() for _ in range(10)]
        return s, out

    a, xa = run(lambda: RayGroupManager(_cfg(), data, KEYS, 24, 8, rank=rank, world=world))
    c, xc = run(lambda: CameraRayGroupManager(_cfg(), gold["cams"], gold["rgba"], gold["modes"], KEYS, 24, 8, rank=rank,
                                              world=world))
    assert len(xa) == len(xc) == 30
    for x, y in zip(xa, xc):
        _same(x, y)
        assert "uncert_masks" in y
    assert not bool(xc[0]["uncert_masks"].any()) and bool(xc[-1]["uncert_masks"].any())
    assert torch.equal(a.uncert_data_idxs, c.uncert_data_idxs) and torch.equal(a.cert_data_idxs, c.cert_data_idxs)
    assert a.stats() == c.stats() and 0 < c.cert_data_num < n
    assert _bits(a.uncert("viewdirs"), c.uncert("viewdirs")) and _bits(a.cert("rgbs"), c.cert("rgbs"))
    # a key the camera set does not provide must be attached before sampling: a message, not a bare KeyError
    extra = CameraRayGroupManager(_cfg(), gold["cams"], gold["rgba"], gold["modes"], KEYS + ["em_colors"], 24, 8)
    with pytest.raises(KeyError, match="set_rows"):
        extra.sample()
    extra.set_rows("em_colors", torch.arange(4, device=DEV), torch.ones(4, 2, device=DEV), fill=0)
    assert extra.sample()["em_colors"].shape == (24, 2)
    # an array attached under a key replaces the camera set's value for it, as on the array manager
    rows = c.uncert_data_idxs[:40]
    vals = torch.arange(40, device=DEV) + 2
    for s in (a, c):
        s.set_rows("em_modes", rows, vals, fill=0)
    torch.manual_seed(2)
    x = a.sample()
    torch.manual_seed(2)
    _same(x, c.sample())


def test_filter_on_cameras_equals_filter_on_their_rays():
    from esr_nerf_amd.camera import Cameras, camera_rays, filter_camera_rays
    from esr_nerf_amd.rayfilter import filter_rays
    poses, K, w, h = CR.filter_set()
    cams = Cameras.from_intrinsics(poses, K, w, h, device=DEV)
    ro, rd, _ = camera_rays(cams)
    for mi, fixed in ((0, True), (1, True), (1, False)):
        m = R.renderers(DEV)[mi]
        want, want_first = filter_rays(m, ro, rd, fixed, want_first_hit=True)
        keep, first = filter_camera_rays(m, cams, fixed, want_first_hit=True)
        assert keep.dtype == torch.bool and keep.shape == (cams.n_rays,) and first.dtype == torch.int32
        assert torch.equal(keep, want) and torch.equal(first, want_first), (mi, fixed)
        assert torch.equal(filter_camera_rays(m, cams, fixed), want)
        share = float(keep.float().mean())
        print(f"model {mi} fixed {fixed}: kept share {share:.3f}")
        assert 0.0 < share < 1.0


def test_frustum_bbox(gold, small):
    from esr_nerf_amd.camera import camera_rays, frustum_bbox
    for cams, blocks in ((gold["cams"], 2), (small, 1)):
        assert -(-cams.n_rays // 256) == blocks                     # below and above one workgroup's share of rays
        for near, far in ((2.0, 6.0), (0.05, 1.7)):
            ro, _, vd = camera_rays(cams)
            pts = torch.stack([ro + vd * near, ro + vd * far])
            lo, hi = frustum_bbox(cams, near, far)
            tol = 2 * U * (float(ro.abs().max()) + far)
            assert lo.shape == hi.shape == (3,) and lo.dtype == torch.float32
            assert float((lo - pts.amin((0, 1))).abs().max()) <= tol and float((hi - pts.amax((0, 1))).abs().max()) <= tol
            assert bool((lo < hi).all())


def test_render_camera_view_equals_render_view_on_the_views_rays():
    from esr_nerf_amd.camera import Cameras, camera_rays
    from esr_nerf_amd.evaluate import render_camera_view, render_view
    poses, K, w, h = CR.filter_set()
    cams = Cameras.from_intrinsics(poses, K, w, h, device=DEV)
    fine = R.renderers(DEV)[1]
    fine.s_val = R.slab().s_val
    fine.eval()
    pos = torch.eye(3, device=DEV)
    view = 1
    ro, rd, vd = camera_rays(cams, view)
    want = render_view(fine, ro, rd, vd, 1, pos, h, w, 200)
    got = render_camera_view(fine, cams, view, 1, pos, 200)
    assert list(got) == list(want) and len(got) > 0
    for k in want:
        assert got[k].shape[:2] == (h, w) and _bits(got[k], want[k]), k
