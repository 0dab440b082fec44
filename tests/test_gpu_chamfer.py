"""The DTU Chamfer metric on the HIP path (esr_nerf_amd/chamfer.py over csrc/chamfer.hip): sampling, the radius
downsample and nearest-neighbour distances bit for bit against the numpy restatement tests/chamfer_ref.py, the metric
against the reference's own DTU_CD (tests/golden/dtu_cd_small.npz), analytic geometry, and a DTU-scale case."""
import math
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chamfer_ref
from conftest import load_npz
from esr_nerf_amd import chamfer, mesh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@torch.no_grad()
def _sphere_mesh(R=40, r=0.6, c=(0.03, -0.02, 0.01), scale=10.0):
    ax = torch.linspace(-1.0, 1.0, R, device=DEV)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    u = (r - ((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2).sqrt()).float().contiguous()
    v, f = mesh.marching_cubes(u, 0.0)
    return ((v / (R - 1) * 2.0 - 1.0) * scale).cpu().numpy(), f.cpu().numpy()


def _random_triangles(n=600, seed=0):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-3, 3, (3 * n, 3))
    f = np.arange(3 * n).reshape(n, 3)
    v[3:30:3] = v[4:31:3] + 1e-9 * rng.standard_normal((9, 3))          # slivers: p0 next to p1
    v[32:60:3] = v[31:59:3] + 0.01 * (v[30:58:3] - v[31:59:3])           # near-collinear
    f[100] = [f[100, 0], f[100, 1], f[100, 0]]                           # zero area: repeated corner
    v[303:305] = np.round(v[303:305])
    v[305] = 2 * v[304] - v[303]                                         # zero area: exactly collinear (integer grid)
    v[400:403] = v[400] + np.array([[0, 0, 0], [5, 0, 0], [0, 0.02, 0]])  # n1 = 0 / n2 = 0 shapes
    v[500:503] = v[500] + np.array([[0, 0, 0], [0.01, 0, 0], [0, 4, 0]])
    return v, f


def test_sampling_is_bit_exact_on_marching_cubes_meshes():
    for R, scale in ((40, 10.0), (24, 12.0)):
        v, f = _sphere_mesh(R, scale=scale)
        v = np.concatenate([v, [[50.0, 50.0, 50.0]]])                    # an unreferenced vertex
        got = chamfer.sample_mesh_points(v, f, 0.2).cpu().numpy()
        want = chamfer_ref.sample_points(v, f, 0.2)
        assert got.shape == want.shape and got.shape[0] > len(v)
        assert np.array_equal(got, want)


def test_sampling_is_bit_exact_on_random_triangles_with_slivers_and_degenerates():
    for seed in range(2):
        v, f = _random_triangles(seed=seed)
        for thresh in (0.2, 0.05):
            got = chamfer.sample_mesh_points(torch.as_tensor(v, device=DEV), torch.as_tensor(f, device=DEV),
                                             thresh).cpu().numpy()
            want = chamfer_ref.sample_points(v, f, thresh)
            assert got.shape == want.shape
            assert np.array_equal(got, want)


def _cloud(n, seed, step=0.25):
    """points on a 1/64 grid with exact duplicates and pairs exactly `step` apart (representable: the boundary case)"""
    rng = np.random.default_rng(seed)
    p = np.round(rng.uniform(0, 4, (n, 3)) * 64) / 64
    p[n // 2:n // 2 + 50] = p[:50]
    p[n // 2 + 50:n // 2 + 100] = p[50:100] + np.array([step, 0, 0])
    return p


def _check_invariants(data, keep, thresh):
    t2 = thresh * thresh
    kept = data[keep]
    dk = chamfer_ref.d2(kept, kept)
    np.fill_diagonal(dk, np.inf)
    assert (dk > t2).all(), "two kept points within thresh"
    ranks = np.flatnonzero(keep)
    for k in np.flatnonzero(~keep):
        near = chamfer_ref.d2(data[k:k + 1], kept)[0] <= t2
        assert (ranks[near] < k).any(), f"removed point {k} has no earlier kept point within thresh"


def test_downsample_equals_the_sequential_loop():
    cases = [(_cloud(4000, 0), 0.25), (_cloud(3000, 1, step=0.125), 0.125)]
    v, f = _sphere_mesh(40, scale=8.0)
    cases.append((chamfer_ref.sample_points(v, f, 0.2), 0.2))
    for pts, thresh in cases:
        n = len(pts)
        for order in (np.arange(n), np.random.default_rng(n).permutation(n)):
            data = pts[order]
            want = chamfer_ref.downsample(data, thresh)
            keep, rounds = chamfer.radius_downsample(torch.as_tensor(pts, device=DEV), thresh, order=order,
                                                     return_rounds=True)
            keep = keep.cpu().numpy()
            assert rounds >= 1
            assert np.array_equal(keep, want)
            _check_invariants(data, keep, thresh)


def test_downsample_of_a_long_chain_in_identity_order():
    # points 0.15 apart on a line at thresh 0.2: each decision waits for the previous one (a chain of n)
    n = 20000
    p = np.zeros((n, 3))
    p[:, 0] = np.arange(n) * 0.15
    keep = chamfer.radius_downsample(torch.as_tensor(p, device=DEV), 0.2).cpu().numpy()
    assert np.array_equal(keep, np.arange(n) % 2 == 0)


def test_nn_is_bit_exact_against_brute_force():
    rng = np.random.default_rng(3)
    d = rng.standard_normal((5000, 3))
    targets = d / np.linalg.norm(d, axis=1, keepdims=True) * 5.0 + 0.01 * rng.standard_normal((5000, 3))
    targets = np.concatenate([targets, rng.uniform(-30, 30, (200, 3)), targets[:10]])   # outliers, duplicates
    queries = np.concatenate([rng.uniform(-6, 6, (3000, 3)), rng.uniform(-60, 60, (1000, 3)), targets[:50]])
    for max_dist in (20.0, 1.0, 0.05):
        want = chamfer_ref.nn(queries, targets, max_dist)
        assert np.isinf(want).any() or max_dist == 20.0
        for cell in (None, 0.2, 0.7, 4.0):
            got = chamfer.nn_distance(torch.as_tensor(queries, device=DEV), targets, max_dist, cell=cell).cpu().numpy()
            assert np.array_equal(got, want), (max_dist, cell)


def test_nn_with_an_empty_and_a_one_point_target_set():
    rng = np.random.default_rng(4)
    q = rng.uniform(-10, 10, (500, 3))
    got = chamfer.nn_distance(torch.as_tensor(q, device=DEV), np.zeros((0, 3)), 20.0).cpu().numpy()
    assert got.shape == (500,) and np.isinf(got).all()
    t = np.array([[1.25, -2.5, 3.0]])
    got = chamfer.nn_distance(torch.as_tensor(q, device=DEV), t, 12.0).cpu().numpy()
    assert np.array_equal(got, chamfer_ref.nn(q, t, 12.0))
    assert np.isinf(got).any() and np.isfinite(got).any()
    assert chamfer.nn_distance(torch.zeros(0, 3, dtype=torch.float64, device=DEV), t).numel() == 0


def test_nn_of_degenerate_target_sets_is_exact_and_quick():
    # a target set of zero extent (one point at the origin, coincident points) or a tiny cluster beside one far point:
    # the cell size comes from max_dist there, not from the extent, and every query walks a few rings at most
    rng = np.random.default_rng(5)
    q = np.concatenate([rng.uniform(-30, 30, (2000, 3)), rng.uniform(-1e-3, 1e-3, (200, 3)), np.zeros((1, 3)),
                        [1.0, 2.0, 3.0] + rng.uniform(-1e-3, 1e-3, (50, 3)),
                        [[5.0, 0.0, 0.0], [0.0, 0.0, -19.999], [400.0, 0.0, 0.0]]])
    sets = [np.zeros((1, 3)), np.zeros((1000, 3)), np.tile([[1.0, 2.0, 3.0]], (1000, 1)),
            np.concatenate([rng.normal(0.0, 1e-6, (5000, 3)), [[1000.0, 0.0, 0.0]]])]
    qd = torch.as_tensor(q, device=DEV)
    chamfer.nn_distance(qd, sets[0], 20.0)                                # warm-up (library load, first launches)
    torch.cuda.synchronize()
    for t in sets:
        for max_dist in (20.0, 0.05):
            t0 = time.perf_counter()
            got = chamfer.nn_distance(qd, t, max_dist).cpu().numpy()
            wall = time.perf_counter() - t0
            assert wall < 2.0, (len(t), max_dist, wall)
            assert np.array_equal(got, chamfer_ref.nn(q, t, max_dist)), (len(t), max_dist)
            assert np.isfinite(got).any()


def _golden_args(z):
    return (z["vertices"], z["triangles"], z["obs_mask"], z["bb"], z["res"], z["stl"], z["plane"], float(z["max_dist"]),
            int(z["patch"]), float(z["thresh"]))


def test_dtu_chamfer_matches_the_reference_golden():
    z = load_npz("dtu_cd_small.npz")
    got = chamfer.dtu_chamfer(*_golden_args(z), order=z["perm"])
    for g, k in zip(got, ("mean_d2s", "mean_s2d", "overall")):
        assert g == pytest.approx(float(z[k]), rel=1e-12, abs=0), k
    # the downsample, exactly: the restatement's keep mask
    _, d = chamfer_ref.dtu_cd(*_golden_args(z)[:7], z["perm"], *_golden_args(z)[7:], detail=True)
    pts = chamfer.sample_mesh_points(z["vertices"], z["triangles"], float(z["thresh"]))
    keep = chamfer.radius_downsample(pts, float(z["thresh"]), order=z["perm"]).cpu().numpy()
    assert np.array_equal(keep, d["keep"])


def test_DTU_CD_drop_in_leaves_the_mesh_alone_and_is_reproducible():
    z = load_npz("dtu_cd_small.npz")
    a = _golden_args(z)
    m = SimpleNamespace(vertices=z["vertices"].copy(), faces=z["triangles"].copy())
    r1 = chamfer.DTU_CD(m, *a[2:7], max_dist=a[7], patch=a[8], thresh=a[9])
    assert np.array_equal(m.vertices, z["vertices"]) and np.array_equal(m.faces, z["triangles"])
    r2 = chamfer.DTU_CD((z["vertices"], z["triangles"]), *a[2:7], max_dist=a[7], patch=a[8], thresh=a[9])
    r3 = chamfer.dtu_chamfer(*a, seed=0)
    assert r1 == r2 == r3                                               # identical floats, run to run
    assert r1[0] == pytest.approx(float(z["mean_d2s"]), rel=0.2)        # another shuffle: close, not equal
    assert chamfer.dtu_chamfer(*a, seed=5) == chamfer.dtu_chamfer(*a, seed=5)
    # nothing selected: nan, as numpy's mean of an empty array
    empty = np.zeros_like(z["obs_mask"])
    d2s, s2d, overall = chamfer.dtu_chamfer(*a[:2], empty, *a[3:], seed=0)
    assert math.isnan(d2s) and math.isnan(overall) and math.isfinite(s2d)


def test_sphere_against_a_dense_analytic_cloud():
    r, n = 50.0, 400_000
    v, f = _sphere_mesh(160, r=0.5, c=(0.0, 0.0, 0.0), scale=2 * r)   # radius 50 mm, 1.26 mm cells
    rng = np.random.default_rng(7)
    d = rng.standard_normal((n, 3))
    stl = d / np.linalg.norm(d, axis=1, keepdims=True) * r
    obs = np.ones((60, 60, 60), bool)
    bb = np.array([[-60.0, -60.0, -60.0], [60.0, 60.0, 60.0]])
    d2s, s2d, overall = chamfer.DTU_CD((v, f), obs, bb, np.array([[2.0]]), stl, np.array([0.0, 0.0, 1.0, 100.0]))
    # data -> stl: a point on the surface to the nearest of n uniform points: 1 / (2 sqrt(density)) for a Poisson
    # process; the marching-cubes chords are within 0.01 mm of the sphere at this resolution
    expect = 0.5 / math.sqrt(n / (4 * math.pi * r * r))
    assert d2s == pytest.approx(expect, rel=0.05)
    assert 0.0 < s2d < 0.2                                           # the downsample keeps a point within 0.2 of each
    assert overall == pytest.approx((d2s + s2d) / 2, rel=1e-15)


def test_extract_geometry_of_a_VoxurfF_model_goes_straight_into_DTU_CD():
    from esr_nerf_amd.config import fine_cfg
    from esr_nerf_amd.synthetic import init_slab_model, slab_scene
    from esr_nerf_amd.voxurff import VoxurfF
    sc = slab_scene("g16")
    torch.manual_seed(0)
    m = VoxurfF(fine_cfg(DEV), sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max,
                sc.mask_alpha_init, sc.mask_density, sc.s_val, sc.num_voxels)
    m = init_slab_model(m, sc)
    ws = [int(x) for x in m.world_size]
    ax = [torch.linspace(float(m.xyz_min[a]), float(m.xyz_max[a]), ws[a], dtype=torch.float64) for a in range(3)]
    X, Y, Z = torch.meshgrid(*ax, indexing="ij")
    c, r = (0.1, -0.05, 0.0), 0.5
    with torch.no_grad():
        m.sdf.grid.copy_((((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2).sqrt() - r).float()[None, None])
    v, f = m.extract_geometry(resolution=128)
    rng = np.random.default_rng(0)
    d = rng.standard_normal((200_000, 3))
    stl = np.asarray(c) + d / np.linalg.norm(d, axis=1, keepdims=True) * r
    lo, hi = m.xyz_min.cpu().numpy(), m.xyz_max.cpu().numpy()
    cell = float((hi - lo).max()) / 127
    stl = stl[((stl > lo + 2 * cell) & (stl < hi - 2 * cell)).all(1)]      # the part of the sphere inside the box
    bb = np.stack([lo, hi]).astype(np.float64)
    res = np.array([[0.05]])
    shape = tuple(int((hi[a] - lo[a]) / 0.05) + 1 for a in range(3))
    d2s, s2d, overall = chamfer.DTU_CD((v, f), np.ones(shape, bool), bb, res, stl, np.array([0.0, 0.0, 1.0, 10.0]),
                                       max_dist=0.5, patch=1, thresh=0.005)
    assert 0.0 < d2s < cell and 0.0 < s2d < cell and math.isfinite(overall)


def test_dtu_scale_case_is_exact_and_fast():
    from scipy.spatial import cKDTree
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import cd_time
    c = cd_time.dtu_case(device=DEV)
    t0 = time.perf_counter()
    ms, st, means = cd_time.run_stages(c)
    wall = time.perf_counter() - t0
    assert wall < 120.0, (wall, ms)
    assert st["points"] > 2_000_000 and st["stl_above"] > 2_000_000 and st["rounds"] >= 1

    # the downsample of the same order, checked: kept points pairwise farther than thresh, removed ones near a kept one
    dev = c["vertices"].device
    pts = chamfer.sample_mesh_points(c["vertices"], c["triangles"], cd_time.THRESH)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    data = pts[torch.randperm(pts.shape[0], generator=g, device=dev)].contiguous()
    keep = chamfer.radius_downsample(data, cd_time.THRESH)
    kept, removed = data[keep].cpu().numpy(), data[~keep].cpu().numpy()
    assert len(kept) == st["kept"]
    tree = cKDTree(kept)
    dk, _ = tree.query(kept, k=2, workers=16)
    assert (dk[:, 1] > cd_time.THRESH * (1 - 1e-12)).all()
    sub = removed[np.random.default_rng(0).choice(len(removed), min(len(removed), 500_000), replace=False)]
    dr, _ = tree.query(sub, k=1, workers=16)
    assert (dr <= cd_time.THRESH * (1 + 1e-12)).all()

    # the means against a kd-tree
    data_in, data_in_obs = chamfer.dtu_filters(data[keep], c["obs_mask"], c["bb"], c["res"], cd_time.PATCH)
    stl = c["stl"]
    stl_above = stl[chamfer.above_plane(torch.as_tensor(stl, device=dev), c["plane"]).cpu().numpy()]
    # (only d < max_dist enters a mean; the bound also spares the kd-tree its slow walks for far outliers)
    d_a, _ = cKDTree(stl).query(data_in_obs.cpu().numpy(), k=1, workers=16, distance_upper_bound=cd_time.MAX_DIST)
    d_b, _ = cKDTree(data_in.cpu().numpy()).query(stl_above, k=1, workers=16, distance_upper_bound=cd_time.MAX_DIST)
    want = (d_a[d_a < cd_time.MAX_DIST].mean(), d_b[d_b < cd_time.MAX_DIST].mean())
    assert means[0] == pytest.approx(want[0], rel=1e-9) and means[1] == pytest.approx(want[1], rel=1e-9)
