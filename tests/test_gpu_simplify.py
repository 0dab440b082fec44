"""mesh.simplify / simplify_to / sources.simplify_surface on the device against tests/simplify_ref.py.

Exact equality with the restatement: cluster keys, the cluster of every vertex, vertex_map, triangles', face_origin and which
clusters survive.  Per value, nothing exempted (simplify_ref.check): the ten quadric numbers, S, W and xbar of EVERY cluster
against exact rational arithmetic, every position, every attribute; and all of them equal the binary64 emulation of the
kernel's order of operations bit for bit.  Every kernel output is allocated with guard bytes on
both sides and at a pointer that is 8- but not 16-byte aligned, the inputs are views at an offset, and they are compared
with their copies afterwards; two runs give the same bytes.  The worst ratios are printed (-s): K_FAMILY comes from them."""
import math

import numpy as np
import pytest
import torch

import simplify_ref as sr
from conftest import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAM = 1e-3
GUARD, FILL = 64, 0xA5
_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


class Guarded:
    """allocator for mesh._simplify(alloc=...): every buffer sits between GUARD bytes of FILL, 8 bytes past a 16-byte boundary"""

    def __init__(self):
        self.buffers = []

    def __call__(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        raw = torch.full((GUARD + 8 + n + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        assert raw.data_ptr() % 16 == 0
        self.buffers.append((raw, n))
        return raw[GUARD + 8: GUARD + 8 + n].view(dtype).reshape(shape)

    def check(self):
        assert len(self.buffers) >= 6
        for raw, n in self.buffers:
            assert bool((raw[:GUARD + 8] == FILL).all()) and bool((raw[GUARD + 8 + n:] == FILL).all()), (n, len(self.buffers))


def shifted(x, dtype):
    """a device copy of x that starts one row into its allocation, and that copy's clone"""
    x = np.ascontiguousarray(x)
    buf = torch.zeros((x.shape[0] + 1,) + x.shape[1:], dtype=dtype, device=DEV)
    buf[1:] = torch.from_numpy(x).to(DEV)
    return buf[1:], buf[1:].clone()


def simplify_checked(what, v, t, h, attr, ex, big=None):
    """runs mesh.simplify on guarded buffers and shifted inputs, holds it to the restatement, returns the worst ratios"""
    from esr_nerf_amd import mesh
    dv, dv0 = shifted(v, torch.float64)
    dt, dt0 = shifted(t, torch.int64)
    da, da0 = shifted(attr, torch.float32) if attr is not None else (None, None)
    guard = Guarded()
    out = mesh._simplify(dv, dt, h, LAM, da, big, debug=True, alloc=guard)
    torch.cuda.synchronize()
    guard.check()
    assert torch.equal(dv, dv0) and torch.equal(dt, dt0) and (da is None or torch.equal(da, da0))
    nv, nt, na, vmap, origin, dbg = out
    assert (nv.dtype, nt.dtype, vmap.dtype, origin.dtype) == (torch.float64, torch.int64, torch.int32, torch.int64)
    assert nv.is_cuda and nt.is_cuda and vmap.is_cuda and origin.is_cuda and (na is None) == (attr is None)
    n_k = len(ex.keys)
    # exact equality
    assert np.array_equal(dbg["cluster_keys"].cpu().numpy(), ex.keys) and np.array_equal(dbg["vertex_cluster"].cpu().numpy(), ex.vc)
    assert np.array_equal(dbg["origin"].cpu().numpy(), ex.origin)
    tri_ref, origin_ref, new_id = sr.faces(ex.vc, t, n_k)
    assert np.array_equal(nt.cpu().numpy(), tri_ref) and tuple(nt.shape) == (len(tri_ref), 3)
    assert np.array_equal(origin.cpu().numpy(), origin_ref)
    assert np.array_equal(vmap.cpu().numpy(), new_id[ex.vc]) and np.array_equal(dbg["used"].cpu().numpy() != 0, new_id >= 0)
    pos, sums = dbg["positions"].cpu().numpy(), dbg["sums"].cpu().numpy()
    live = new_id >= 0
    assert np.array_equal(nv.cpu().numpy().view(np.int64), pos[live].view(np.int64)) and tuple(nv.shape) == (int(live.sum()), 3)
    all_attr = None
    if attr is not None:
        all_attr = dbg["attr"].cpu().numpy()
        assert na.dtype == torch.float32 and np.array_equal(na.cpu().numpy().view(np.int32), all_attr[live].view(np.int32))
    # per value
    worst, fails = sr.check(ex, dict(sums=sums[:, :12], xbar=sums[:, 12:], pos=pos, attr=all_attr), what,
                            mesh.SIMPLIFY_BIG if big is None else big)
    print(f"  {what:34s} K {n_k:5d} F' {len(tri_ref):5d} " + " ".join(f"{k} {x:.3f}" for k, x in worst.items()))
    assert not fails, fails[:5]
    # bit for bit the binary64 emulation of the kernel's order of operations
    em = sr.emulate(v, t, h, LAM, attr, mesh.SIMPLIFY_BIG if big is None else big)
    assert np.array_equal(em["sums"].view(np.int64), sums[:, :12].view(np.int64))
    assert np.array_equal(em["xbar"].view(np.int64), sums[:, 12:].view(np.int64)) and np.array_equal(em["pos"].view(np.int64), pos.view(np.int64))
    assert attr is None or np.array_equal(em["attr"].view(np.int32), all_attr.view(np.int32))
    # every new vertex in its cell's box: y is clamped to it, then g + y is rounded once
    hh = 0.5 * h
    assert (np.abs(pos - ex.g) <= hh + 2.0 ** -52 * (np.abs(ex.g) + hh)).all()
    # the same bytes again, and the same without the debug output and on torch's own allocations
    again = mesh._simplify(dv, dt, h, LAM, da, big, debug=True)
    plain = mesh.simplify(dv, dt, h, lam=LAM, attr=da, big=big)
    assert len(plain) == 5
    for a, b, c in zip(out[:5], again[:5], plain):
        assert (a is None and b is None and c is None) or (torch.equal(a, b) and torch.equal(a, c) and a.shape == c.shape)
    assert all(torch.equal(dbg[k], again[5][k]) for k in ("sums", "positions", "used", "cluster_keys", "vertex_cluster"))
    assert all(np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)) for x, y in
               ((dbg["sums"], again[5]["sums"]), (nv, plain[0])))
    return worst, out


def mc_sphere():
    """the marching-cubes sphere of a 24^3 field, about 3 k faces, in a box of side 2"""
    def build():
        from esr_nerf_amd import mesh
        ax = torch.arange(24, dtype=torch.float32, device=DEV)
        x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
        u = 9.3 - torch.sqrt((x - 11.3) ** 2 + (y - 11.6) ** 2 + (z - 11.45) ** 2)
        v, t = mesh.marching_cubes(u.contiguous())
        v, t = v.cpu().numpy() * (2.0 / 23.0) - 1.0, t.cpu().numpy()
        assert 2000 < len(t) < 4000 and v.dtype == np.float64
        return v, t
    return memo("mc_sphere", build)


VOXEL = 2.0 / 23.0


@pytest.mark.parametrize("cells,n_c", [(2.5, 12), (4.0, 1), (7.3, 0)])
def test_marching_cubes_sphere(cells, n_c):
    v, t = mc_sphere()
    h = cells * VOXEL
    attr = sr.attributes(v, n_c, seed=7) if n_c else None
    ex = memo(("sphere", cells), lambda: sr.exact(v, t, h, LAM, attr))
    _, out = simplify_checked(f"mc sphere h = {cells} voxels C = {n_c}", v, t, h, attr, ex)
    nv, nt = out[0].cpu().numpy(), out[1].cpu().numpy()
    # clustering may pinch a surface in general; this sphere stays closed at all three cell sizes: every edge lies in two
    # faces and the Euler characteristic is 2
    e = np.sort(np.concatenate([nt[:, [0, 1]], nt[:, [1, 2]], nt[:, [2, 0]]]), 1)
    ue, cnt = np.unique(e, axis=0, return_counts=True)
    print(f"  faces {len(t)} -> {len(nt)}, vertices {len(v)} -> {len(nv)}, radius {np.linalg.norm(nv - nv.mean(0), axis=1).min():.4f} .. "
          f"{np.linalg.norm(nv - nv.mean(0), axis=1).max():.4f} (input {9.3 * VOXEL:.4f}), Euler {len(nv) - len(ue) + len(nt)}, "
          f"edges not in two faces {int((cnt != 2).sum())}")
    assert len(nt) < len(t) / 4 and len(nt) > 20
    assert (cnt == 2).all() and len(nv) - len(ue) + len(nt) == 2


def test_big_threshold_moves_only_the_order_of_the_sums():
    """the sphere at 4 voxels with every cluster on the workgroup path (big = 1), a mix (big = 24) and the default: the
    integer outputs are equal, every value is inside its bound on each path, and a fixed big gives the same bytes"""
    v, t = mc_sphere()
    h = 4.0 * VOXEL
    attr = sr.attributes(v, 1, seed=7)
    ex = memo(("sphere", 4.0), lambda: sr.exact(v, t, h, LAM, attr))
    assert min(ex.n_pairs) <= 24 < max(ex.n_pairs)
    outs = [simplify_checked(f"mc sphere h = 4 voxels big = {big}", v, t, h, attr, ex, big)[1] for big in (1, 24, None)]
    for o in outs[1:]:
        assert torch.equal(o[1], outs[0][1]) and torch.equal(o[3], outs[0][3]) and torch.equal(o[4], outs[0][4])
        assert float((o[0] - outs[0][0]).abs().max()) <= 2 * sr.K_FAMILY["pos"] * sr.U * (1 + 1 / LAM) * h


def test_cube_with_sharp_edges():
    v, t = sr.cube(8)
    v = v + 0.0137
    attr = sr.attributes(v, 3, seed=1)
    h = 0.29
    ex = sr.exact(v, t, h, LAM, attr)
    _, out = simplify_checked("cube", v, t, h, attr, ex)
    # the plane quadrics keep the flat sides flat: where every incident face of a cluster lies in one plane of the cube, A has
    # rank one, the mean lies in that plane and so does the new vertex (the regulariser only moves it within the plane)
    pos = out[5]["positions"].cpu().numpy()
    inc = sr.incident(ex.vc, t)
    flat = 0
    for k, fs in enumerate(inc):
        corners = v[t[fs]].reshape(-1, 3)
        for a in range(3):
            if np.ptp(corners[:, a]) == 0.0:
                flat += 1
                assert abs(pos[k, a] - corners[0, a]) <= 4 * sr.U * (abs(corners[0, a]) + h), (k, a)
    print(f"  cube: {flat} of {len(inc)} clusters lie in one side")
    assert flat == 24


@pytest.mark.parametrize("name", sr.EDGE_CASES)
def test_exact_edge_cases(name):
    v, t, h = sr.edge_case(name)
    attr = sr.attributes(v, 4, seed=2)
    ex = sr.exact(v, t, h, LAM, attr)
    _, out = simplify_checked(name, v, t, h, attr, ex)
    if name in ("one_cell", "no_faces"):
        assert out[0].shape == (0, 3) and out[1].shape == (0, 3) and out[2].shape == (0, 4) and out[4].shape == (0,)
        assert bool((out[3] == -1).all())
    if name == "two_sheets":
        assert out[4].tolist() == [0, 3]
    if name == "all_degenerate_cluster":
        k = int(ex.vc[3])
        assert np.array_equal(out[5]["attr"][k].cpu().numpy(), attr[3]) and float(out[5]["sums"][k, 10]) == 0.0


def test_one_cluster_of_twenty_thousand_faces_takes_the_workgroup_path():
    """19 602 faces on 10 000 vertices in one cell: 77 trips of the strided partial sums over the pairs, 40 over the members"""
    v, t = sr.dense_patch(100)
    attr = sr.attributes(v, 2, seed=5)
    ex = sr.exact(v, t, 1.0, LAM, attr)
    assert len(ex.keys) == 1 and ex.n_pairs[0] == 19602 > 2 * sr.THREADS and ex.n_members[0] == 10000
    _, out = simplify_checked("one cluster, 19 602 faces", v, t, 1.0, attr, ex)
    assert out[1].shape == (0, 3)


def test_empty_mesh_and_refusals():
    from esr_nerf_amd import mesh
    f64, i64 = dict(dtype=torch.float64, device=DEV), dict(dtype=torch.int64, device=DEV)
    out = mesh.simplify(torch.zeros(0, 3, **f64), torch.zeros(0, 3, **i64), 0.5)
    assert [tuple(x.shape) for x in out if x is not None] == [(0, 3), (0, 3), (0,), (0,)] and out[2] is None
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.5, 0.25], [0.5, 1.0, 0.75]], **f64)
    t = torch.tensor([[0, 1, 2]], **i64)
    bad = v.clone()
    bad[1, 2] = math.inf

    def wide(x):
        w = v.clone()
        w[1, 0] = float(x)
        return w
    for fn in (lambda: mesh.simplify(bad, t, 0.5), lambda: mesh.simplify(v * math.nan, t, 0.5),
               lambda: mesh.simplify(v, t, 0.0), lambda: mesh.simplify(v, t, -1.0), lambda: mesh.simplify(v, t, math.nan),
               lambda: mesh.simplify(wide(2 ** 21 - 1), t, 1.0),                       # cells 0 .. 2^21 - 1: one too many on x
               lambda: mesh.simplify(v, t, 0.5, lam=0.0), lambda: mesh.simplify(v, t, 0.5, big=0),
               lambda: mesh.simplify(v, t + 1, 0.5), lambda: mesh.simplify(v.float(), t, 0.5),
               lambda: mesh.simplify(v, t.int(), 0.5), lambda: mesh.simplify(v, t, 0.5, attr=torch.zeros(3, 17, device=DEV)),
               lambda: mesh.simplify(v, t, 0.5, attr=torch.zeros(2, 3, device=DEV)),
               lambda: mesh.simplify(v, t, 0.5, attr=torch.zeros(3, 3, dtype=torch.float64, device=DEV)),
               lambda: mesh.simplify_to(v, t, -1), lambda: mesh.simplify_to(v, t, 1, max_trials=25),
               lambda: mesh.simplify_to(v, t, 1, cell_min=0.0)):
        with pytest.raises(ValueError):
            fn()
    nv, nt, na, vmap, origin = mesh.simplify(wide(2 ** 21 - 2), t, 1.0)               # the widest grid an axis holds
    assert nt.tolist() == [[0, 2, 1]] and vmap.tolist() == [0, 2, 1] and na is None and origin.tolist() == [0]
    assert float((nv - wide(2 ** 21 - 2)[[0, 2, 1]]).abs().max()) <= 1.0              # clusters by ascending key: x first


def test_simplify_to_brackets_the_target():
    from esr_nerf_amd import mesh
    v, t = mc_sphere()
    dv, dt = torch.from_numpy(v).to(DEV), torch.from_numpy(t).to(DEV)
    attr = torch.from_numpy(sr.attributes(v, 3, seed=7)).to(DEV)
    for target in (300, 40):
        out, cell, over = mesh.simplify_to(dv, dt, target, attr=attr)
        assert out[1].shape[0] <= target and over is not None and over < cell
        assert mesh.simplify(dv, dt, over)[1].shape[0] > target
        direct = mesh.simplify(dv, dt, cell, attr=attr)
        assert all(torch.equal(a, b) for a, b in zip(out, direct))
        assert cell <= over * 1.02 or out[1].shape[0] == target
        print(f"  simplify_to({target}): {len(t)} -> {out[1].shape[0]} faces at cell {cell:.5f}, {over:.5f} leaves more")
    out, cell, over = mesh.simplify_to(dv, dt, len(t))                               # the lower end already meets it
    assert over is None and out[1].shape[0] <= len(t) and cell == float(np.linalg.norm(v.max(0) - v.min(0))) / 2 ** 20
    out, cell, over = mesh.simplify_to(dv, dt, 300, max_trials=3)
    assert out[1].shape[0] <= 300 and over is not None


# ----------------------------------------------------------------------------------------------------------------------
# end to end on the g16 model: extract_surface -> simplify_surface -> emissive_sources -> rasterize -> edit_view_data -> PLY


def test_end_to_end_on_the_g16_model(tmp_path):
    from esr_nerf_amd import chamfer, mesh, raster
    from esr_nerf_amd.camera import Cameras
    from esr_nerf_amd.config import lts_cfg
    from esr_nerf_amd.esrnerf import ESRNeRF
    from esr_nerf_amd.sources import emissive_sources, extract_surface, simplify_surface, write_surface_ply
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
    rep = emissive_sources(surf, k_val)
    v, t = surf.vertices, surf.triangles
    extent = float((v.amax(0) - v.amin(0)).max())
    h = 2.5 * extent / 47.0
    # The old surface as a point set: chamfer.sample_mesh_points at a spacing of h / 16 and, so that the set's spacing is
    # proven, the lattice points p0 + (i v1 + j v2) / N of every face, i + j <= N: they cut the face into N^2 copies of
    # itself at scale 1 / N, and a point of a triangle is within its longest edge of one of its corners, so every point of
    # the old surface lies within (the longest old edge) / N of the set.
    N = 16
    longest = float(torch.stack([(v[t[:, a]] - v[t[:, b]]).norm(dim=1) for a, b in ((0, 1), (1, 2), (2, 0))]).max())
    ij = torch.tensor([(i, j) for i in range(N + 1) for j in range(N + 1 - i)], dtype=torch.float64, device=DEV) / N
    p0, v1, v2 = v[t[:, 0]], v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
    lattice = (p0[:, None] + ij[None, :, :1] * v1[:, None] + ij[None, :, 1:] * v2[:, None]).reshape(-1, 3)
    old_surface = torch.cat([chamfer.sample_mesh_points(v, t, thresh=h / 16), lattice]).contiguous()
    slack = longest / N
    assert slack < 0.05 * h
    for kw in (dict(model=m), dict()):
        small, fs = simplify_surface(surf, cell=h, face_source=rep.face_source, **kw)
        nv, nt, na, vmap, origin = mesh.simplify(v, t, h)
        assert torch.equal(small.vertices, nv) and torch.equal(small.triangles, nt) and torch.equal(fs, rep.face_source[origin])
        assert 20 < nt.shape[0] < t.shape[0] // 3 and fs.dtype == torch.int32
        assert set(small.attrs) == set(surf.attrs)
        for k, x in small.attrs.items():
            assert x.dtype == torch.float32 and x.shape == (nv.shape[0],) + tuple(surf.attrs[k].shape[1:]) and bool(torch.isfinite(x).all())
        assert float((small.attrs["normal"].norm(dim=1) - 1).abs().max()) < 1e-5
        # A point sum_i l_i y_i of a new face lies within h sqrt 3 of the point sum_i l_i a_i of the face it came from, y_i
        # and a_i sharing a cell: every sample of the new surface is within h sqrt 3 of the old surface, and so within
        # h sqrt 3 + slack of the point set that stands for it.
        pts = chamfer.sample_mesh_points(small.vertices, small.triangles, thresh=h / 4)
        d = chamfer.nn_distance(pts, old_surface, max_dist=4 * h)
        print(f"  g16 ({'re-queried' if kw else 'area-weighted'}): {t.shape[0]} -> {nt.shape[0]} faces, {pts.shape[0]} samples against "
              f"{old_surface.shape[0]} points of the old surface, worst distance {float(d.max()) / h:.3f} h "
              f"(bound {math.sqrt(3) + slack / h:.3f} h)")
        assert float(d.max()) <= h * math.sqrt(3) + slack
        rep2 = emissive_sources(small, k_val)
        assert rep2.face_source.shape == (nt.shape[0],)
        centre = v.mean(0).cpu().numpy()
        eye = centre + 3.0 * extent * np.asarray([0.4, -0.5, 1.0]) / np.linalg.norm([0.4, -0.5, 1.0])
        z = (eye - centre) / np.linalg.norm(eye - centre)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        P = np.eye(4)
        P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, np.cross(z, x), z, eye
        cams = Cameras.from_blender(P[None], 2.0 * np.arctan(0.5 / 1.4), 33, 33, device=DEV)
        r = raster.rasterize(small.vertices, small.triangles, cams)
        seen, seen0 = int((r.face >= 0).sum()), int((raster.rasterize(v, t, cams).face >= 0).sum())
        print(f"  the view sees the surface in {seen0} pixels and the simplified one in {seen}")
        assert seen0 > 100 and seen0 // 2 < seen < 2 * seen0 and int(r.face.max()) < nt.shape[0]
        if len(rep2):
            td = raster.edit_view_data(small, rep2, cams, 0, [dict(sources=[0], mode="off")])
            assert tuple(td["em_masks"].shape) == (1, 33, 33)
        path = str(tmp_path / "small.ply")
        write_surface_ply(path, small, fs)
        pv, pf = chamfer.read_ply(path)
        assert np.array_equal(pv, nv.cpu().numpy()) and np.array_equal(pf, nt.cpu().numpy())
    small, fs = simplify_surface(surf, target_faces=200, face_source=rep.face_source)
    assert 0 < small.triangles.shape[0] <= 200 and fs.shape == (small.triangles.shape[0],)
