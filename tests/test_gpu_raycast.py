"""raycast.build / cast / occluded / occluded_segments / cast_cameras and sources.source_visibility on the device against
tests/raycast_ref.py.

The build: keys, sorted order, child and parent links and every box equal to the restatement, exactly.  The walk: the face
equal on every unambiguous ray and inside the accepted set on the others, t and the barycentrics bit-equal to the binary64
emulation of the kernel's order of operations and inside |x - x_ref| <= K_T 2^-53 absref against extended precision.  Every
kernel output is allocated between guard bytes at a pointer that is 8- (nodes: 16-) but not 32-byte aligned; one case runs
on inputs that start one row into their allocation; two runs give the same bytes.  The worst ratios are printed (-s): K_T
comes from them."""
import math

import numpy as np
import pytest
import torch

import raycast_ref as rr
import raster_ref
from conftest import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, FILL = 64, 0xA5
_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


class Guarded:
    """allocator for raycast._build / _cast(alloc=...): every buffer sits between GUARD bytes of FILL, 8 bytes (node
    records: 16) past a 32-byte boundary"""

    def __init__(self):
        self.buffers = []

    def __call__(self, shape, dtype):
        shape = tuple(shape) if isinstance(shape, (tuple, list)) else (shape,)
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        off = 16 if (len(shape) == 2 and shape[1] == 16 and dtype == torch.int32) else 8
        raw = torch.full((GUARD + off + n + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        assert raw.data_ptr() % 32 == 0
        self.buffers.append((raw, n, off))
        return raw[GUARD + off: GUARD + off + n].view(dtype).reshape(shape)

    def check(self, at_least):
        assert len(self.buffers) >= at_least
        for raw, n, off in self.buffers:
            assert bool((raw[:GUARD + off] == FILL).all()) and bool((raw[GUARD + off + n:] == FILL).all()), (n, len(self.buffers))


def shifted(x, dtype):
    """a device copy of x that starts one row into its allocation, and that copy's clone"""
    x = np.ascontiguousarray(x)
    buf = torch.zeros((x.shape[0] + 1,) + x.shape[1:], dtype=dtype, device=DEV)
    buf[1:] = torch.from_numpy(x).to(DEV)
    return buf[1:], buf[1:].clone()


def dev(x, dtype=None):
    t = torch.from_numpy(np.array(x, order="C")).to(DEV)
    return t if dtype is None else t.to(dtype)


def mc_sphere():
    """the marching-cubes sphere of test_gpu_simplify.py: a 24^3 field, 3 216 faces, in a box of side 2"""
    def build():
        from esr_nerf_amd import mesh
        ax = torch.arange(24, dtype=torch.float32, device=DEV)
        x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
        u = 9.3 - torch.sqrt((x - 11.3) ** 2 + (y - 11.6) ** 2 + (z - 11.45) ** 2)
        v, t = mesh.marching_cubes(u.contiguous())
        v, t = v.cpu().numpy() * (2.0 / 23.0) - 1.0, t.cpu().numpy()
        assert len(t) == 3216 and v.dtype == np.float64
        return v, t
    return memo("mc_sphere", build)


MESHES = {"faces0": lambda: (np.zeros((3, 3)), np.zeros((0, 3), np.int64)), "faces1": lambda: rr.few_faces(1),
          "faces2": lambda: rr.few_faces(2), "faces3": lambda: rr.few_faces(3), "lumpy": rr.lumpy_sphere, "mc": mc_sphere,
          "twins": rr.twins, "nan_vertex": rr.with_nan_vertex, "chain": rr.chain, "far_small": rr.far_small,
          "room": lambda: rr.room()[:2]}


def mesh_of(name):
    return memo(("mesh", name), MESHES[name])


def bvh_of(name):
    from esr_nerf_amd import raycast
    return memo(("bvh", name), lambda: raycast.build(dev(mesh_of(name)[0]), dev(mesh_of(name)[1])))


# ----------------------------------------------------------------------------------------------------------------------
# the build


@pytest.mark.parametrize("name", list(MESHES))
def test_build_equals_the_restatement(name):
    from esr_nerf_amd import raycast
    v, tr = mesh_of(name)
    T, nb, fb, k = rr.built(v, tr)
    dv, dv0 = shifted(v, torch.float64)
    dt, dt0 = shifted(tr, torch.int64)
    guard = Guarded()
    b = raycast._build(dv, dt, alloc=guard)
    torch.cuda.synchronize()
    guard.check(6)
    assert torch.equal(dv.view(torch.int64), dv0.view(torch.int64)) and torch.equal(dt, dt0)      # (bytes: a NaN equals itself)
    n = len(tr)
    assert np.array_equal(b.scene_box.cpu().numpy(), rr.scene_box(v))
    assert np.array_equal(b.keys.cpu().numpy(), T.skeys) and np.array_equal(b.order.cpu().numpy(), T.order)
    assert np.array_equal(b.face_boxes.cpu().numpy().view(np.int32), fb.view(np.int32))
    words = b.nodes.cpu().numpy()
    want = rr.node_words(T, nb)
    assert words.shape == (max(n - 1, 0), 16) and b.nodes.dtype == torch.int32
    assert np.array_equal(words[:, 12:], want[:, 12:]), "child, parent, pad"
    assert np.array_equal(words[:, :12], want[:, :12]), "boxes"
    if n > 1:
        assert np.array_equal(b.leaf_parent.cpu().numpy(), T.leaf_parent)
    assert np.array_equal(b.root_box.cpu().numpy().view(np.int32), T.root_box.view(np.int32))
    if name == "chain":
        assert T.depth > 64
    again = raycast.build(dv, dt)
    for x, y in ((b.nodes, again.nodes), (b.order, again.order), (b.keys, again.keys), (b.face_boxes, again.face_boxes),
                 (b.root_box, again.root_box), (b.leaf_parent, again.leaf_parent)):
        assert x.shape == y.shape and np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    print(f"  {name:12s} F {n:5d} depth {T.depth}")


# ----------------------------------------------------------------------------------------------------------------------
# the walk


def cases():
    def make():
        out = rr.sphere_cases("lumpy", *mesh_of("lumpy"))
        out.update(rr.sphere_cases("mc", *mesh_of("mc")))
        out.update(rr.other_cases(4096))
        out.update(rr.room_cases())
        return out
    return memo("cases", make)


CASE_NAMES = tuple(f"{m}/{c}" for m in ("lumpy", "mc") for c in ("generic_cam", "inside_cam", "axis", "special", "interval", "skip")) + \
    ("chain/random", "twins/random", "far_small/along_y", "nan_vertex/generic_cam", "faces1/random", "faces2/random",
     "faces3/random", "room/axis")


def case_ref(name):
    return memo(("ref", name), lambda: rr.case_brute(cases()[name]))


def run_case(c, bvh, any_hit=False, stats=False, shift=False, sl=slice(None)):
    """one guarded call of the C entry on the rays ``sl`` of a case -> numpy results"""
    from esr_nerf_amd import raycast
    n_all = len(c["o"])
    o, d = c["o"][sl], c["d"][sl]
    n = len(o)
    if shift:
        (do, do0), (dd, dd0) = shifted(o, torch.float64), shifted(d, torch.float64)
    else:
        do, dd = dev(o), dev(d)

    def interval(x, default):
        x = c.get(x, default)
        return dev(np.broadcast_to(np.asarray(x, np.float64), (n_all,))[sl]) if isinstance(x, np.ndarray) else float(x)
    lo, hi = interval("t_min", 0.0), interval("t_max", math.inf)
    skip = dev(np.asarray(c["skip"], np.int32)[sl]) if "skip" in c else None
    guard = Guarded()
    out = raycast._cast("test", bvh, do, dd, lo, hi, skip, any_hit, stats, alloc=guard)
    torch.cuda.synchronize()
    guard.check(1 if any_hit else 3)
    if shift:
        assert torch.equal(do, do0) and torch.equal(dd, dd0)
    return [None if x is None else x.cpu().numpy() for x in out]


def check_case(name, c, ref, bvh, shift=False):
    face, t, bary, _ = run_case(c, bvh, shift=shift)
    assert face.dtype == np.int32 and t.dtype == np.float64 and bary.shape == (len(face), 2)
    share = rr.check_hits(ref, face, t, bary, name)
    same = (face == ref["face"]) & (face >= 0)
    # bit for bit the binary64 emulation of the kernel's order of operations
    assert np.array_equal(t[same].view(np.int64), ref["t"][same].view(np.int64)), name
    assert np.array_equal(bary[same, 0].view(np.int64), ref["u"][same].view(np.int64)), name
    assert np.array_equal(bary[same, 1].view(np.int64), ref["v"][same].view(np.int64)), name
    assert (bary[face < 0] == 0).all()
    rt = rr.t_ratio(c["v"], c["tr"], c["o"], c["d"], ref, face, t)
    rb = rr.bary_ratio(c["v"], c["tr"], c["o"], c["d"], ref, face, bary[:, 0], bary[:, 1])
    print(f"  {name:26s} rays {len(face):6d} hit {int((face >= 0).sum()):6d} ambiguous {int(ref['ambiguous'].sum()):4d} "
          f"worst t {rt:.3f} bary {rb:.3f} of K_T = {rr.K_T}")
    assert rt <= rr.K_T and rb <= rr.K_T, (name, rt, rb)
    assert rt <= rr.K_T_WORST, "the recorded worst ratio is the worst"
    if c.get("generic"):
        assert share < 0.01
    # the same bytes again
    again = run_case(c, bvh)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip((face, t, bary), again[:3]))
    # any hit: the nearest mode's face >= 0 on every unambiguous ray
    hit, _ = run_case(c, bvh, any_hit=True, shift=shift)
    clear = ~ref["ambiguous"]
    assert hit.dtype == np.uint8 and np.array_equal(hit[clear] != 0, ref["hit"][clear]) and set(np.unique(hit)) <= {0, 1}
    assert np.array_equal(hit != 0, face >= 0), "the two modes walk the same boxes and test the same faces"
    return face, t


@pytest.mark.parametrize("name", CASE_NAMES)
def test_nearest_and_any_hit(name):
    assert set(CASE_NAMES) == set(cases())
    c, ref = cases()[name], case_ref(name)
    face, t = check_case(name, c, ref, bvh_of(name.split("/")[0]), shift=name == "lumpy/inside_cam")
    if name == "twins/random":                                      # twins have the same t to the bit: the smaller id
        assert np.array_equal(face, ref["face"]) and (face[face >= 0] < 500).all()
    if name.endswith("/skip"):
        assert (face != c["skip"]).all() and (face >= 0).all()
    if name == "nan_vertex/generic_cam":
        v, tr = mesh_of("nan_vertex")
        assert np.isfinite(v[tr[face[face >= 0]]]).all()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_ray_counts_around_a_wave(n):
    c, ref = cases()["lumpy/generic_cam"], case_ref("lumpy/generic_cam")
    sl = slice(500, 500 + n)
    face, t, bary, _ = run_case(c, bvh_of("lumpy"), sl=sl)
    assert len(face) == n and np.array_equal(face, ref["face"][sl]) and np.array_equal(t, ref["t"][sl])
    hit, _ = run_case(c, bvh_of("lumpy"), any_hit=True, sl=sl)
    assert np.array_equal(hit != 0, ref["hit"][sl])
    if n == 65:
        assert 0 < int((face >= 0).sum()) < n


def test_a_second_trip_of_the_grid_stride():
    """2048 workgroups of 256 lanes make one trip of 524 288 rays: 65 more than that, on three faces"""
    v, tr = mesh_of("faces3")
    n = 2048 * 256 + 65
    o, d = rr.rays_at_faces(v, tr, n, seed=5, radius=3.0)
    c = dict(v=v, tr=tr, o=o, d=d)
    ref = rr.case_brute(c)
    face, t, bary, _ = run_case(c, bvh_of("faces3"))
    rr.check_hits(ref, face, t, bary, "second trip")
    same = face == ref["face"]
    assert same.mean() > 0.999 and np.array_equal(t[same], ref["t"][same]) and (face[-65:] >= 0).all()


def test_float32_rays_are_widened_exactly_and_empty_mesh_hits_nothing():
    from esr_nerf_amd import raycast
    c = cases()["lumpy/generic_cam"]
    o32, d32 = c["o"].astype(np.float32), c["d"].astype(np.float32)
    ref = rr.brute(c["v"], c["tr"], o32.astype(np.float64), d32.astype(np.float64))
    h = raycast.cast(bvh_of("lumpy"), dev(o32), dev(d32))
    clear = ~ref["ambiguous"]
    assert np.array_equal(h.face.cpu().numpy()[clear], ref["face"][clear])
    same = h.face.cpu().numpy() == ref["face"]
    assert np.array_equal(h.t.cpu().numpy()[same], ref["t"][same])
    e = raycast.cast(bvh_of("faces0"), dev(c["o"]), dev(c["d"]))
    assert bool((e.face == -1).all()) and bool(torch.isposinf(e.t).all())
    assert not bool(raycast.occluded(bvh_of("faces0"), dev(c["o"]), dev(c["d"]), 0.0, math.inf).any())
    for bad in (lambda: raycast.cast(bvh_of("lumpy"), dev(o32), dev(d32)[:5]), lambda: raycast.cast(bvh_of("lumpy"), dev(o32).cpu(), dev(d32)),
                lambda: raycast.cast(bvh_of("lumpy"), dev(o32), dev(d32), skip_face=torch.zeros(3, dtype=torch.int32, device=DEV))):
        with pytest.raises(ValueError):
            bad()


def test_occluded_segments_between_sphere_vertices():
    from esr_nerf_amd import raycast
    v, tr = mesh_of("lumpy")
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, len(v), 600), rng.integers(0, len(v), 600)
    keep = a != b
    p, q = v[a[keep]], v[b[keep]]
    # skip one face at the far vertex (the others that meet there are hit at t = 1 > 1 - eps, or not at all)
    skip = np.array([int(np.flatnonzero((tr == x).any(1))[0]) for x in b[keep]], np.int32)
    eps = 1e-4                                                      # (the faces that meet at p lie at t = 0 to rounding)
    ref = rr.brute(v, tr, p, q - p, eps, 1.0 - eps, skip)
    occ = raycast.occluded_segments(bvh_of("lumpy"), dev(p), dev(q), skip_face=dev(skip), eps=eps).cpu().numpy()
    clear = ~ref["ambiguous"]
    assert occ.dtype == np.uint8 and clear.mean() > 0.9 and np.array_equal(occ[clear] != 0, ref["hit"][clear])
    assert 0 < int(occ.sum()) < len(occ)
    v2, tr2, p2, q2, eps = rr.segment_case()
    assert not bool(raycast.occluded_segments(bvh_of("lumpy"), dev(p2), dev(q2), eps=eps).any())
    assert bool(raycast.occluded_segments(bvh_of("lumpy"), dev(p2), dev(q2), eps=0.0).all())


def test_the_walk_prunes():
    """The mean number of triangles tested per ray on the 3 216-face sphere from the generic camera is below F / 16 = 201:
    a linear scan cannot pass as a BVH.  Measured: 0.82 triangles and 20.05 boxes per ray (every ray, the three quarters that miss the sphere included)."""
    c = cases()["mc/generic_cam"]
    face, t, bary, stats = run_case(c, bvh_of("mc"), stats=True)
    assert stats.dtype == np.int32 and stats.shape == (len(face), 2) and (stats >= 0).all()
    print(f"  boxes per ray {stats[:, 0].mean():.2f}, triangles per ray {stats[:, 1].mean():.2f}, most {stats.max(0)}")
    assert stats[:, 1].mean() < len(c["tr"]) / 16
    assert (stats[face >= 0, 1] >= 1).all()


# ----------------------------------------------------------------------------------------------------------------------
# against the rasteriser


@pytest.mark.parametrize("name", ["lumpy", "mc"])
def test_cast_cameras_against_the_rasteriser(name):
    from esr_nerf_amd import raster, raycast
    from esr_nerf_amd.camera import Cameras
    cam = raster_ref.generic_cam()
    cams = Cameras(torch.from_numpy(cam.poses).to(DEV), cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)
    v, tr = mesh_of(name)
    face, depth = raycast.cast_cameras(bvh_of(name), cams)
    r = raster.rasterize(dev(v), dev(tr), cams)
    assert int(r.n_dropped.sum()) == 0
    assert face.shape == r.face.shape == (3, cam.height, cam.width) and depth.dtype == torch.float64
    ref = case_ref(f"{name}/generic_cam")
    clear = ~ref["ambiguous"]
    f0, f1 = face.cpu().numpy().reshape(-1), r.face.cpu().numpy().reshape(-1)
    assert np.array_equal(f0[clear], ref["face"][clear]) and np.array_equal(f1[clear], ref["face"][clear])
    d0, d1 = depth.cpu().numpy().reshape(-1), r.depth.cpu().numpy().reshape(-1)
    same = clear & (f0 >= 0)
    assert np.array_equal(np.isposinf(d0), f0 < 0)
    err = np.abs(d0[same].astype(np.float32).astype(np.float64) - d1[same].astype(np.float64))
    assert (err <= np.spacing(d1[same]).astype(np.float64)).all(), "float32(depth) within one rounding of the rasteriser's"
    one = raycast.cast_cameras(bvh_of(name), cams, views=1)
    assert torch.equal(one[0], face[1:2]) and torch.equal(one[1], depth[1:2])


# ----------------------------------------------------------------------------------------------------------------------
# source_visibility


class Report:
    def __init__(self, face_source, n):
        self.face_source, self.n = face_source, n

    def __len__(self):
        return self.n


@pytest.mark.parametrize("samples", [1, 16, 100])
def test_source_visibility_in_the_room(samples):
    from esr_nerf_amd import raycast, sources
    v, tr, fs, S = rr.room()
    pts = rr.room_points()
    surf = sources.Surface(dev(v), dev(tr), {})
    rep = Report(dev(fs), S)
    bvh = bvh_of("room")
    share_ref, bits, amb = rr.visibility(v, tr, fs, S, pts, samples)
    assert amb == 0
    faces, points, margin = rr.source_samples(v, tr, fs, S, samples)
    face, point, n = sources.source_samples(surf, rep, samples)
    for s in range(S):
        k = len(faces[s])
        assert int(n[s]) == k and np.array_equal(face[s, :k].cpu().numpy(), faces[s])
        assert np.array_equal(point[s, :k].cpu().numpy(), points[s])
        occ = raycast.occluded_segments(bvh, dev(np.repeat(pts, k, 0)), dev(np.tile(points[s], (len(pts), 1))),
                                        skip_face=dev(np.tile(faces[s], len(pts)).astype(np.int32)))
        assert np.array_equal(occ.cpu().numpy().reshape(len(pts), k), bits[s]), "every segment's bit"
    for b in (bvh, None):
        share = sources.source_visibility(surf, rep, dev(pts), samples=samples, bvh=b)
        assert share.dtype == torch.float32 and share.shape == (len(pts), S)
        assert np.array_equal(share.cpu().numpy().view(np.int32), share_ref.view(np.int32))
    assert np.array_equal(sources.source_visibility(surf, rep, dev(pts).float(), samples=samples, bvh=bvh).cpu().numpy(),
                          rr.visibility(v, tr, fs, S, pts.astype(np.float32), samples)[0])
    if samples == 16:
        assert share_ref[0, 0] == 0.0 and share_ref[2, 0] > 0.0 and (share_ref[5] == 0.0).all()
        assert tuple(sources.source_visibility(surf, Report(dev(fs) * 0 - 1, 0), dev(pts), bvh=bvh).shape) == (len(pts), 0)
        assert tuple(sources.source_visibility(surf, rep, dev(pts)[:0], bvh=bvh).shape) == (0, S)
        old = sources.VISIBILITY_CHUNK
        sources.VISIBILITY_CHUNK = 70                               # three launches instead of one
        try:
            assert np.array_equal(sources.source_visibility(surf, rep, dev(pts), samples=16, bvh=bvh).cpu().numpy(), share_ref)
        finally:
            sources.VISIBILITY_CHUNK = old


def test_end_to_end_on_the_g16_model():
    from esr_nerf_amd import raycast
    from esr_nerf_amd.config import lts_cfg
    from esr_nerf_amd.esrnerf import ESRNeRF
    from esr_nerf_amd.sources import emissive_sources, extract_surface, simplify_surface, source_visibility
    from esr_nerf_amd.synthetic import slab_scene
    sc = slab_scene("g16", s_val=60.0, oblique=True, n_rays=1920, seed=0)
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = lts_cfg(DEV, num_2ndrays=8, num_ltspts=12)
    m = ESRNeRF(cfg, sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max, sc.mask_alpha_init,
                sc.mask_density, sc.s_val, sc.num_voxels)
    m.load_state_dict({k: torch.from_numpy(x).to(DEV) for k, x in load_npz("lts_g16_params.npz").items()})
    m.s_val = 60.0
    m.eval()
    surf = extract_surface(m, resolution=48)
    k_val = float(surf.attrs["emission"].max(dim=1).values.median())
    v = surf.vertices
    h = 2.5 * float((v.amax(0) - v.amin(0)).max()) / 47.0
    small, _ = simplify_surface(surf, cell=h, face_source=emissive_sources(surf, k_val).face_source)
    rep = emissive_sources(small, k_val)
    S = len(rep)
    assert S >= 1 and small.triangles.shape[0] > 20
    bvh = raycast.build(small.vertices, small.triangles)
    vis = source_visibility(small, rep, small.vertices, bvh=bvh)
    assert vis.shape == (small.vertices.shape[0], S) and vis.dtype == torch.float32
    assert bool(torch.isfinite(vis).all()) and float(vis.min()) >= 0.0 and float(vis.max()) <= 1.0
    assert torch.equal(vis, source_visibility(small, rep, small.vertices))
    nv, nt, fs = small.vertices.cpu().numpy(), small.triangles.cpu().numpy(), rep.face_source.cpu().numpy()
    sub = np.linspace(0, len(nv) - 1, 257).astype(np.int64)
    ref, _, amb = rr.visibility(nv, nt, fs, S, nv[sub], 16)
    _, _, margin = rr.source_samples(nv, nt, fs, S, 16)
    got = vis.cpu().numpy()[sub]
    print(f"  g16: {nt.shape[0]} faces, {S} sources, {len(nv)} points; mean visibility {got.mean():.4f}; of the subset's "
          f"{257 * S * 16} segments (at most) {amb} are ambiguous; sample margin {margin:.2e}")
    assert np.array_equal(got, ref)
