"""The surface rasteriser on the device (esr_nerf_amd/csrc/raster.hip, raster.py) against the ray-casting restatement of
tests/raster_ref.py, through the Python API and the raw C ABI.

``face`` must EQUAL the restatement on every unambiguous pixel and lie in the acceptable set on the others; ``depth``,
where both name the same face, is one rounding of the float64 ray parameter: |depth - t| <= 2^-24 t (1 + 2^-20);
``depth`` is +inf exactly where ``face`` is -1; ``n_dropped`` is exact.  The z-buffer words do not depend on ``big_px``
(which path rasterised a face), on the run, or on how the views were chunked.  On every generic case the restatement sets
aside at most 0.5 % of the pixels (the shares are printed).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import raster_ref as rr
from conftest import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8
Z_NEAR = 1e-6
CAP = 0.005
# the launchers' caps (csrc/raster.hip): RS_BLOCKS x RS_THREADS lanes per trip of the per-(view, face) and per-pixel
# launches, RS_LARGE_BLOCKS queue entries per trip of the large-face launch
TRIP, LARGE_TRIP = 1024 * 256, 512
_memo = {}


def memo(key, fn):
    """references are computed once and shared (never modified)"""
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def dev(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def cameras(cam):
    from esr_nerf_amd.camera import Cameras
    return Cameras(torch.from_numpy(cam.poses).to(DEV), cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)


def run(v, t, cam, **kw):
    from esr_nerf_amd import raster
    r = raster.rasterize(dev(v, torch.float64).reshape(-1, 3), dev(t, torch.int64).reshape(-1, 3), cameras(cam), **kw)
    assert r.face.dtype == torch.int32 and r.depth.dtype == torch.float32 and r.n_dropped.dtype == torch.int32
    assert r.face.is_cuda and r.depth.is_cuda and r.n_dropped.is_cuda
    return r


def same(a, b):
    # (depth compared as bits: -0 / NaN could not hide a difference)
    return torch.equal(a.face, b.face) and torch.equal(a.depth.view(torch.int32), b.depth.view(torch.int32)) and \
        torch.equal(a.n_dropped, b.n_dropped)


def check(name, v, t, cam, r, refs, cap=CAP):
    face, depth = r.face.cpu().numpy(), r.depth.cpu().numpy()
    assert face.shape == depth.shape == (len(refs), cam.height, cam.width)
    assert r.n_dropped.cpu().tolist() == [ref["n_dropped"] for ref in refs], name
    amb = 0
    worst = 0.0
    for view, ref in enumerate(refs):
        share, w = rr.check_against(ref, face[view], depth[view], (name, view))
        amb += int(ref["ambiguous"].sum())
        worst = max(worst, w)
    n = len(refs) * cam.width * cam.height
    print(f"{name}: {int((face >= 0).sum())} covered of {n} pixels, {amb} ambiguous ({amb / n:.2%}), "
          f"largest depth error / bound {worst:.3f}, dropped {r.n_dropped.cpu().tolist()}")
    if cap is not None:
        assert amb <= cap * n, (name, amb, n)
    return face, depth


def every_path_and_chunking(v, t, cam, r):
    """the same words whichever path rasterised a face, on a second run and for every chunking of the views"""
    from esr_nerf_amd import raster
    for kw in (dict(big_px=0), dict(big_px=2 ** 30), dict()):
        assert same(run(v, t, cam, **kw), r), kw
    per_view, whole = 8 * (cam.width * cam.height + len(t)), raster.CHUNK_BYTES
    try:
        for views_per_chunk, big in ((1, None), (2, 3)):
            raster.CHUNK_BYTES = views_per_chunk * per_view
            assert same(run(v, t, cam, big_px=big), r), views_per_chunk
    finally:
        raster.CHUNK_BYTES = whole
    part = raster.rasterize(dev(v, torch.float64).reshape(-1, 3), dev(t, torch.int64).reshape(-1, 3), cameras(cam), views=(1, 3))
    assert torch.equal(part.face, r.face[1:3]) and torch.equal(part.n_dropped, r.n_dropped[1:3])
    one = raster.rasterize(dev(v, torch.float64).reshape(-1, 3), dev(t, torch.int64).reshape(-1, 3), cameras(cam), views=2)
    assert torch.equal(one.depth.view(torch.int32), r.depth[2:3].view(torch.int32))


# ----------------------------------------------------------------------------------------------------------------------
# meshes


def mesh_case(name):
    def build():
        cam = rr.generic_cam()
        if name in ("outside", "inside", "twins", "pixel"):
            v, t = rr.lumpy_sphere()
            if name == "inside":
                cam = rr.inside_cam()
            if name == "twins":
                t = np.concatenate([t, t[::-1]], 0)
            if name == "pixel":
                cam = rr.Cam(cam.poses, 30.0, 28.0, 0.4, 0.6, 1, 1)
        elif name == "marching_cubes":
            from esr_nerf_amd import mesh
            n = 24
            vi, ti = mesh.marching_cubes(torch.from_numpy(rr.blob_field(n)).to(DEV), 0.0)
            v, t = vi.cpu().numpy() / (n - 1) * 2.0 - 1.0, ti.cpu().numpy()
        elif name == "giant":
            # the sphere in front of ONE triangle far larger than the image: its vertices project ~1e6 pixels outside
            v, t = rr.lumpy_sphere()
            m = cam.poses[0].astype(np.float64)
            at = lambda x, y, z: m[:, 3] + m[:, 0] * x + m[:, 1] * y + m[:, 2] * z
            big = np.stack([at(-2e5, -1.5e5, 6.0), at(2.2e5, -1.1e5, 7.0), at(1e4, 2.4e5, 5.5)])
            v, t = np.concatenate([v, big]), np.concatenate([t, [[len(v), len(v) + 1, len(v) + 2]]])
        elif name == "large300":
            # 300 big triangles through the unit ball: every one covers hundreds of pixels, they cut each other
            rng = np.random.default_rng(3)
            v = rng.uniform(-1.3, 1.3, (900, 3))
            t = np.arange(900).reshape(300, 3)
        elif name == "near":
            # the sphere, a face straddling z_near of view 0 (centroid in front), three faces behind the camera of view 0
            v, t = rr.lumpy_sphere()
            m = cam.poses[0].astype(np.float64)
            at = lambda x, y, z: m[:, 3] + m[:, 0] * x + m[:, 1] * y + m[:, 2] * z
            extra = [at(-0.5, -0.4, 1.0), at(0.6, -0.3, 1.2), at(0.0, 0.5, -0.5)]
            for k in range(3):
                extra += [at(-0.3 + k, -0.2, -1.0 - k), at(0.4, -0.3 + k, -1.5), at(0.0, 0.5, -2.0 - k)]
            n0 = len(v)
            v, t = np.concatenate([v, np.stack(extra)]), np.concatenate([t, np.arange(n0, n0 + 12).reshape(4, 3)])
        elif name == "degenerate":
            # in FRONT of the sphere for view 0: a repeated vertex, three collinear points, a sliver, a NaN vertex
            v, t = rr.lumpy_sphere()
            m = cam.poses[0].astype(np.float64)
            at = lambda x, y, z: m[:, 3] + m[:, 0] * x + m[:, 1] * y + m[:, 2] * z
            p, q = at(-0.3, -0.2, 1.5), at(0.4, 0.3, 1.6)
            extra = [p, p, q,
                     at(-0.3, 0.0, 1.5), at(0.0, 0.0, 1.5), at(0.3, 0.0, 1.5),
                     at(-0.31, -0.21, 1.4), at(0.29, 0.33, 1.45), at(0.29 + 1e-9, 0.33 + 1e-9, 1.45),
                     at(-0.2, -0.2, 1.3), at(0.3, -0.1, 1.3), np.array([np.nan, 0.0, 0.0])]
            n0 = len(v)
            v, t = np.concatenate([v, np.stack(extra)]), np.concatenate([t, np.arange(n0, n0 + 12).reshape(4, 3)])
        elif name == "blind":
            # view 1 looks past the sphere (everything in front of it, nothing in the image), view 2 away from it
            v, t = rr.lumpy_sphere()
            cam = rr.Cam([cam.poses[0], rr.look_at((3.2, 0.3, 0.4), (2.787, -0.599, 0.277)), rr.look_at((3.2, 0.3, 0.4), (8.0, 0.3, 0.5))],
                         cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)
        elif name == "strip":
            # more (view, face) pairs than one trip of the launch holds, seen through a 64 x 1 image
            n = 364
            x, y = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n), indexing="ij")
            v = np.stack([x, y, 0.1 * np.sin(5 * x) * np.cos(4 * y)], -1).reshape(-1, 3)
            a = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None, :]).reshape(-1)
            t = np.concatenate([np.stack([a, a + n, a + 1], 1), np.stack([a + 1, a + n, a + n + 1], 1)])
            t = np.stack([t[:len(a)], t[len(a):]], 1).reshape(-1, 3)            # the two faces of a cell side by side
            cam = rr.Cam([rr.look_at((0.93, -0.1, 2.5), (0.95, 0.05, 0.0), up=(0, 1, 0))], 600.0, 630.0, 31.3, 0.4, 64, 1)
        else:
            raise KeyError(name)
        return v, np.asarray(t, np.int64), cam, rr.cast(v, t, cam, Z_NEAR)
    return memo(name, build)


@pytest.mark.parametrize("name", ["outside", "inside", "marching_cubes"])
def test_generic_meshes_equal_the_ray_cast(name):
    v, t, cam, refs = mesh_case(name)
    r = run(v, t, cam)
    face, _ = check(name, v, t, cam, r, refs)
    assert (face >= 0).sum() > 400
    if name == "inside":
        assert min(ref["n_dropped"] for ref in refs) > 50
    every_path_and_chunking(v, t, cam, r)


def test_a_triangle_far_larger_than_the_image():
    v, t, cam, refs = mesh_case("giant")
    r = run(v, t, cam)
    face, _ = check("giant", v, t, cam, r, refs)
    assert (face[0] == len(t) - 1).sum() > 300 and (face[0] >= 0).all()            # it fills what the sphere leaves of view 0
    every_path_and_chunking(v, t, cam, r)


def test_300_large_faces_through_the_queue():
    v, t, cam, refs = mesh_case("large300")
    assert 3 * len(t) > LARGE_TRIP                                                   # a second trip of the large-face launch
    r = run(v, t, cam, big_px=0)
    check("large300", v, t, cam, r, refs)
    every_path_and_chunking(v, t, cam, r)


def test_faces_at_and_behind_the_near_plane_are_dropped_and_counted():
    v, t, cam, refs = mesh_case("near")
    assert refs[0]["n_dropped"] == 4
    r = run(v, t, cam)
    face, _ = check("near", v, t, cam, r, refs)
    assert (face[0] < 288).all()                                                     # nothing of the four dropped faces in view 0
    sphere = mesh_case("outside")
    assert np.array_equal(face[0], run(sphere[0], sphere[1], cam).face[0].cpu().numpy())
    every_path_and_chunking(v, t, cam, r)


def test_identical_faces_the_smaller_id_wins():
    v, t, cam, refs = mesh_case("twins")
    r = run(v, t, cam)
    face, depth = check("twins", v, t, cam, r, refs, cap=None)                       # (every covered pixel is a tie)
    single = run(v, t[:288], cam)
    assert torch.equal(r.face, single.face) and torch.equal(r.depth.view(torch.int32), single.depth.view(torch.int32))
    every_path_and_chunking(v, t, cam, r)


def test_degenerate_faces_cover_nothing_and_harm_nothing():
    v, t, cam, refs = mesh_case("degenerate")
    r = run(v, t, cam)
    face, _ = check("degenerate", v, t, cam, r, refs)
    assert not np.isin(face, [288, 289, 291]).any()                                  # repeated vertex, collinear, NaN
    sphere = mesh_case("outside")
    plain = run(sphere[0], sphere[1], cam).face.cpu().numpy()
    assert np.array_equal(np.where(face == 290, plain, face), plain)                 # but for the sliver's own pixels
    every_path_and_chunking(v, t, cam, r)


def test_views_that_see_nothing_and_empty_meshes():
    v, t, cam, refs = mesh_case("blind")
    r = run(v, t, cam)
    face, depth = check("blind", v, t, cam, r, refs)
    assert (face[1:] == -1).all() and np.isposinf(depth[1:]).all() and (face[0] >= 0).any()
    assert r.n_dropped.cpu().tolist() == [0, 0, 288]
    for vv, tt in ((v, np.zeros((0, 3), np.int64)), (np.zeros((0, 3)), np.zeros((0, 3), np.int64))):
        e = run(vv, tt, cam)
        assert bool((e.face == -1).all()) and bool(torch.isposinf(e.depth).all()) and e.n_dropped.cpu().tolist() == [0, 0, 0]
    from esr_nerf_amd import raster
    none = raster.rasterize(dev(v), dev(t), cameras(cam), views=(2, 2))
    assert none.face.shape == (0, cam.height, cam.width) and none.n_dropped.shape == (0,)
    with pytest.raises(ValueError):
        raster.rasterize(dev(v), dev(np.array([[0, 1, len(v)]])), cameras(cam))
    with pytest.raises(ValueError):
        raster.rasterize(dev(v), dev(t), cameras(cam), views=(2, 4))
    with pytest.raises(ValueError):
        raster.rasterize(dev(v), dev(t), cameras(cam), z_near=0.0)
    with pytest.raises(ValueError):
        raster.rasterize(dev(v).float(), dev(t), cameras(cam))


def test_small_images_and_a_second_trip_of_the_face_launch():
    v, t, cam, refs = mesh_case("strip")
    assert len(t) > TRIP and (cam.width, cam.height) == (64, 1)
    r = run(v, t, cam)
    face, _ = check("strip", v, t, cam, r, refs)
    assert (face >= 0).sum() >= 32 and face.max() > TRIP                             # faces of the second trip are seen
    assert same(run(v, t, cam, big_px=0), r)
    v, t, cam, refs = mesh_case("pixel")
    r = run(v, t, cam)
    check("pixel", v, t, cam, r, refs, cap=None)
    assert r.face.shape == (3, 1, 1) and bool((r.face >= 0).all())


# ----------------------------------------------------------------------------------------------------------------------
# the C ABI: memory discipline, the words themselves, resolve and masks on more than one trip


def guarded(host, off, fill):
    """(buffer, view): `host` copied behind `off` guard elements and in front of GUARD more"""
    host = torch.as_tensor(np.ascontiguousarray(host))
    buf = torch.full((off + host.numel() + GUARD,), fill, dtype=host.dtype, device=DEV)
    view = buf[off: off + host.numel()]
    view.copy_(host.reshape(-1))
    return buf, view


def raw_pipeline(shift, big_px, groups, fs, n_src):
    """every entry through the raw C ABI on guarded buffers `shift` elements off their allocations' bases"""
    from esr_nerf_amd import _lib, raster
    L = _lib.lib()
    v, t, cam, _ = mesh_case("giant")
    cams = cameras(cam)
    n_v, n_f, n_px, nv = len(v), len(t), cam.width * cam.height, cam.n_views
    ins = {"v": (v.astype(np.float64), 3.5), "t": (t.astype(np.int64), 7), "w": (raster.world_to_camera(cams), 2.5),
           "fs": (np.asarray(fs, np.int32), 9), "cond": (raster._conditions(n_src, groups), 11)}
    ibuf = {k: guarded(h, shift, fill) + (h, fill) for k, (h, fill) in ins.items()}
    outs = {}

    def out(name, n, dtype, fill):
        buf = torch.full((shift + n + GUARD,), fill, dtype=dtype, device=DEV)
        outs[name] = (buf, buf[shift: shift + n], fill)
        return C.c_void_p(buf[shift: shift + n].data_ptr())

    def untouched():
        torch.cuda.synchronize()
        return all(bool((buf == fill).all()) for buf, _, fill in outs.values())

    p = lambda k: C.c_void_p(ibuf[k][1].data_ptr())
    s = _lib.stream_ptr(torch.device(DEV))
    cs = cams.struct()
    zbuf, drop = out("zbuf", nv * n_px, torch.int64, -5), out("drop", nv, torch.int32, -5)
    queue, count = out("queue", nv * n_f, torch.int64, -5), out("count", 1, torch.int64, -5)
    face, depth = out("face", nv * n_px, torch.int32, -5), out("depth", nv * n_px, torch.float32, -5.0)
    n_cond = len(groups)
    masks, pixels = out("masks", nv * n_cond * n_px, torch.float32, -5.0), out("pixels", nv * n_src, torch.int64, -5)
    call = lambda **kw: L.esr_raster_faces(*[kw.get(k, d) for k, d in (
        ("cam", C.byref(cs)), ("w", p("w")), ("v0", 0), ("v1", nv), ("v", p("v")), ("nv", n_v), ("t", p("t")), ("nf", n_f),
        ("z_near", Z_NEAR), ("big", big_px), ("zbuf", zbuf), ("drop", drop), ("queue", queue), ("cap", nv * n_f), ("count", count),
        ("s", s))])
    # every refusal leaves the prefill
    for kw in (dict(v1=nv + 1), dict(v0=-1), dict(z_near=0.0), dict(big=-1), dict(nf=-1), dict(zbuf=None), dict(w=None),
               dict(zbuf=C.c_void_p(zbuf.value + 4)), dict(cap=nv * n_f - 1), dict(nf=2 ** 31, cap=2 ** 40)):
        assert call(**kw) in (-1, -2) and untouched(), kw
    assert L.esr_raster_resolve(zbuf, -1, face, depth, s) == -1 and L.esr_raster_resolve(zbuf, 2 ** 31, face, depth, s) == -2
    assert L.esr_source_masks(face, nv, n_px, p("fs"), n_f, p("cond"), n_src, 17, masks, pixels, s) == -2
    assert L.esr_source_masks(face, nv, n_px, p("fs"), n_f, p("cond"), n_src, -1, masks, pixels, s) == -1 and untouched()
    assert call() == 0
    assert L.esr_raster_resolve(zbuf, nv * n_px, face, depth, s) == 0
    assert L.esr_source_masks(face, nv, n_px, p("fs"), n_f, p("cond") if n_src else None, n_src, n_cond, masks,
                              pixels if n_src else None, s) == 0
    torch.cuda.synchronize()
    for name, (buf, view, fill) in outs.items():
        assert bool((buf[:shift] == fill).all()) and bool((buf[shift + view.numel():] == fill).all()), f"{name}: the guard changed"
    for name, (buf, view, h, fill) in ibuf.items():
        assert bool((buf[:shift] == fill).all()) and bool((buf[shift + view.numel():] == fill).all()), f"{name}: an input's guard"
        assert np.array_equal(view.cpu().numpy().view(np.uint8), np.ascontiguousarray(h).reshape(-1).view(np.uint8)), name
    return {name: x[1].cpu().numpy() for name, x in outs.items() if name not in ("queue", "count")}


def test_memory_discipline_shifted_pointers_and_words_that_do_not_depend_on_the_path():
    v, t, cam, refs = mesh_case("giant")
    rng = np.random.default_rng(9)
    n_src = 5
    fs = rng.integers(-1, n_src, len(t)).astype(np.int32)
    fs[-1] = 3                                                                       # the giant triangle is source 3
    groups = [[3, 0], [1]]                                                           # sources 2 and 4 are in no condition
    runs = {(sh, big): raw_pipeline(sh, big, groups, fs, n_src) for sh, big in ((0, 64), (1, 0), (3, 2 ** 30), (2, 64))}
    first = runs[(0, 64)]
    for key, r in runs.items():
        for name in first:
            assert np.array_equal(r[name].view(np.uint8), first[name].view(np.uint8)), (key, name)
    nv, n_px = cam.n_views, cam.width * cam.height
    z = first["zbuf"].view(np.uint64)
    face, depth = first["face"].reshape(nv, cam.height, cam.width), first["depth"].reshape(nv, -1)
    assert np.array_equal(np.where(z == np.uint64(2 ** 64 - 1), -1, (z & np.uint64(0xffffffff)).astype(np.int64)), face.reshape(-1))
    assert np.array_equal((z >> np.uint64(32)).astype(np.uint32)[face.reshape(-1) >= 0], depth.reshape(-1).view(np.uint32)[face.reshape(-1) >= 0])
    for view, ref in enumerate(refs):
        rr.check_against(ref, face[view], depth[view], ("raw", view))
    assert first["drop"].tolist() == [ref["n_dropped"] for ref in refs]
    masks, pixels = rr.source_masks(face, fs, n_src, groups)
    assert np.array_equal(first["masks"].reshape(masks.shape), masks) and np.array_equal(first["pixels"].reshape(pixels.shape), pixels)
    assert masks[0, 0].sum() > 300 and pixels[:, [2, 4]].sum() > 0                   # ungrouped sources are counted, in no mask
    # no sources at all, and no conditions
    for g, n_s in (([], 0), ([[], []], 0), ([], n_src)):
        r = raw_pipeline(1, 64, g, fs if n_s else np.full(len(t), -1, np.int32), n_s)
        assert np.array_equal(r["face"], first["face"])
        m, px = rr.source_masks(face, fs if n_s else np.full(len(t), -1), n_s, g)
        assert np.array_equal(r["masks"].reshape(m.shape), m) and np.array_equal(r["pixels"].reshape(px.shape), px)


def test_resolve_and_masks_on_more_than_one_trip():
    from esr_nerf_amd import _lib, raster
    L = _lib.lib()
    s = _lib.stream_ptr(torch.device(DEV))
    rng = np.random.default_rng(11)
    n_views, n_px, n_f, n_src = 3, TRIP // 2 - 77, 5000, 7                           # 3 views: the last trip is ragged
    n = n_views * n_px
    assert n > TRIP
    face = rng.integers(-1, n_f, n).astype(np.int64)
    bits = rng.integers(1, 0x7f800000, n).astype(np.uint64)
    words = np.where(face >= 0, (bits << np.uint64(32)) | face.astype(np.uint64), np.uint64(2 ** 64 - 1))
    zb = dev(words.view(np.int64))
    f_d, d_d = torch.full((n,), -7, dtype=torch.int32, device=DEV), torch.full((n,), -7.0, device=DEV)
    assert L.esr_raster_resolve(_lib.ptr(zb), n, _lib.ptr(f_d), _lib.ptr(d_d), s) == 0
    assert np.array_equal(f_d.cpu().numpy(), face)
    want = np.where(face >= 0, bits.astype(np.uint32), np.float32(np.inf).view(np.uint32))
    assert np.array_equal(d_d.cpu().numpy().view(np.uint32), want)
    fs = rng.integers(-1, n_src, n_f).astype(np.int32)
    groups = [[6], [0, 2], [5]]
    runs = face.copy()                                                               # long runs of one source beside mixed waves
    runs[1000:200000] = 17
    for fc in (face, runs):
        fimg = dev(fc.reshape(n_views, 1, n_px), torch.int32)
        masks, pixels = raster.source_masks(fimg, dev(fs), n_src, groups)
        m, px = rr.source_masks(fc.reshape(n_views, 1, n_px), fs, n_src, groups)
        assert masks.shape == (n_views, 3, 1, n_px) and pixels.dtype == torch.int64
        assert np.array_equal(masks.cpu().numpy(), m) and np.array_equal(pixels.cpu().numpy(), px)


# ----------------------------------------------------------------------------------------------------------------------
# wiring: extract_surface -> emissive_sources -> rasterize -> edit_view_data -> label_edit_rays / EditRaySelector / FinetuneStep

SIDE = 33                                       # square: label_edit_rays tests both coordinates against both sizes


def wired():
    def build():
        from esr_nerf_amd.camera import Cameras
        from esr_nerf_amd.config import lts_cfg
        from esr_nerf_amd.esrnerf import ESRNeRF
        from esr_nerf_amd.sources import emissive_sources, extract_surface
        from esr_nerf_amd.synthetic import slab_scene
        sc = slab_scene("g16", s_val=60.0, oblique=True, n_rays=1920, seed=0)
        torch.manual_seed(0)
        np.random.seed(0)
        cfg = lts_cfg(DEV, num_2ndrays=8, num_ltspts=12)
        cfg.system["data_preload"] = "cuda"
        m = ESRNeRF(cfg, sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max, sc.mask_alpha_init,
                    sc.mask_density, sc.s_val, sc.num_voxels)
        m.load_state_dict({k: torch.from_numpy(x).to(DEV) for k, x in load_npz("lts_g16_params.npz").items()})
        m.s_val = 60.0
        m.eval()
        surf = extract_surface(m, resolution=48)
        em = surf.attrs["emission"]
        rep = emissive_sources(surf, float(em.max(dim=1).values.median()))
        v, t = surf.vertices.cpu().numpy(), surf.triangles.cpu().numpy()
        centre, extent = v.mean(0), np.abs(v - v.mean(0)).max()
        mats = []
        for off in ([0.4, -0.5, 1.0], [-0.6, 0.3, -0.9]):                            # Blender poses: x right, y up, z backward
            eye = centre + 3.0 * extent * np.asarray(off) / np.linalg.norm(off)
            z = (eye - centre) / np.linalg.norm(eye - centre)
            x = np.cross([0.0, 1.0, 0.0], z)
            x /= np.linalg.norm(x)
            P = np.eye(4)
            P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, np.cross(z, x), z, eye
            mats.append(P)
        angle = 2.0 * np.arctan(0.5 / 1.4)                                           # focal = 1.4 x the width
        cams = Cameras.from_blender(np.stack(mats), angle, SIDE, SIDE, device=DEV)
        cam = rr.Cam(cams.poses.cpu().numpy(), cams.fx, cams.fy, cams.cx, cams.cy, SIDE, SIDE)
        return dict(model=m, sc=sc, cfg=cfg, surf=surf, rep=rep, v=v, t=t, cams=cams, cam=cam, mats=np.stack(mats),
                    refs=rr.cast(v, t, cam, Z_NEAR))
    return memo("wired", build)


def test_wiring_surface_to_edit_labels():
    from esr_nerf_amd import raster
    from esr_nerf_amd.relight import dilate_masks, label_edit_rays
    w = wired()
    surf, rep, cams, cam, refs = w["surf"], w["rep"], w["cams"], w["cam"], w["refs"]
    assert len(w["t"]) > 1000 and len(rep) >= 2
    r = raster.rasterize(surf.vertices, surf.triangles, cams)
    face, _ = check("g16 surface", w["v"], w["t"], cam, r, refs)
    assert (face >= 0).sum() > 400
    _, pixels = raster.source_masks(r.face, rep.face_source, len(rep), [])
    view = 0
    # the two sources of which this view sees the most pixels whose eight neighbours see them too
    fs_h = rep.face_source.cpu().numpy()
    src = np.where(face[view] >= 0, fs_h[np.clip(face[view], 0, None)], -1)
    inner = np.ones((SIDE - 2, SIDE - 2), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            inner &= src[1 + dy:SIDE - 1 + dy, 1 + dx:SIDE - 1 + dx] == src[1:-1, 1:-1]
    counts = np.bincount(src[1:-1, 1:-1][inner & (src[1:-1, 1:-1] >= 0)], minlength=len(rep))
    seen = [int(x) for x in np.argsort(-counts, kind="stable")[:2]]
    assert counts[seen[1]] > 0 and int(pixels[view, seen[1]]) >= counts[seen[1]], counts.tolist()
    edits = [dict(sources=[seen[0]], mode="off"), dict(sources=[seen[1]], mode="i_change", intensity=2.5)]
    td = raster.edit_view_data(surf, rep, cams, view, edits)
    assert np.array_equal(td["poses"].cpu().numpy(), w["mats"][view].astype(np.float32))
    assert td["em_modes"].tolist() == [0, 2] and td["em_intensities"].tolist() == [1.0, 2.5] and tuple(td["em_colors"].shape) == (2, 3)
    fs = rep.face_source.cpu().numpy()
    m_ref, px_ref = rr.source_masks(face[view:view + 1], fs, len(rep), [[seen[0]], [seen[1]]])
    assert np.array_equal(td["em_masks"].cpu().numpy(), m_ref[0]) and np.array_equal(td["source_pixels"].cpu().numpy(), px_ref[0])
    assert int(td["n_dropped"]) == refs[view]["n_dropped"]
    # the labels of the view's own pixels, from the ray cast's hit points
    ref = refs[view]
    masks = dilate_masks(td["em_masks"], 1)
    assert torch.equal(masks, td["em_masks"])
    lab = label_edit_rays(torch.from_numpy(ref["hit"].astype(np.float32)).to(DEV), td["poses"], cams.fx, SIDE, SIDE, masks,
                          td["em_modes"], td["em_intensities"], td["em_colors"])
    lab = {k: x.cpu().numpy() for k, x in lab.items()}
    cond = np.where(m_ref[0, 0] > 0, 0, np.where(m_ref[0, 1] > 0, 1, -1))            # [H, W]
    flat = np.ones((SIDE, SIDE), bool)
    flat[[0, -1], :] = flat[:, [0, -1]] = False
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            flat[1:-1, 1:-1] &= cond[1 + dy:SIDE - 1 + dy, 1 + dx:SIDE - 1 + dx] == cond[1:-1, 1:-1]
    ok = flat.reshape(-1) & ~ref["ambiguous"] & (ref["face"] >= 0)
    c = cond.reshape(-1)
    print(f"labels checked on {int(ok.sum())} pixels: {int((ok & (c == 0)).sum())} off, {int((ok & (c == 1)).sum())} i_change")
    assert (ok & (c == 0)).sum() > 0 and (ok & (c == 1)).sum() > 0 and (ok & (c < 0)).sum() > 100
    assert np.array_equal(lab["keep"][ok], c[ok] >= 0)
    assert np.array_equal(lab["em_modes"][ok], np.where(c == 0, 0, np.where(c == 1, 2, 1))[ok])
    assert np.array_equal(lab["em_intensities"][ok], np.where(c == 1, np.float32(2.5), np.float32(0.0)).astype(np.float32)[ok])


def test_wiring_selector_and_finetune_step_take_the_view_data():
    from esr_nerf_amd import raster
    from esr_nerf_amd.data import RayGroupManager
    from esr_nerf_amd.relight import EditRaySelector, finetune_radiance
    w = wired()
    m, sc, cfg, cams = w["model"], w["sc"], w["cfg"], w["cams"]
    keys = ["rgbs", "rays_o", "rays_d", "viewdirs", "em_modes"]
    perm = torch.randperm(1920, generator=torch.Generator().manual_seed(5))
    s = RayGroupManager(cfg, {k: sc.batch[k] for k in keys}, list(keys), 128, 128, uncert_data_idxs=perm[:1500],
                        cert_data_idxs=perm[1500:])
    state = {k: x.detach().clone() for k, x in m.state_dict().items()}
    sel = EditRaySelector(m, s, cams.fx, (SIDE, SIDE), 5, 500)
    n_src = len(w["rep"])
    td = raster.edit_view_data(w["surf"], w["rep"], cams, 0, [dict(sources=list(range(0, n_src, 2)), mode="off"),
                                                               dict(sources=list(range(1, n_src, 2)), mode="ic_change",
                                                                    intensity=1.5, color=(0.3, 0.6))])
    assert sel.apply(td) is s
    n_keep = int(sel.labels["keep"].sum())
    print(f"the view keeps {n_keep} of 1500 training rays")
    assert set(torch.unique(sel.labels["em_modes"]).tolist()) <= {0, 1, 4}
    try:
        losses = finetune_radiance(m, sel, td, 1, dict(emo_color=0.01, emo_rgbnet=1e-3), 0.5, state=state)
        assert len(losses) == 1 and np.isfinite(losses[0])
    finally:
        m.load_state_dict(state, strict=False)
        for p in m.parameters():
            p.requires_grad_(True)
        m.eval()
