"""Mesh export on the HIP path (esr_nerf_amd/mesh.py over csrc/mesh.hip): the lattice field against the torch
``extract_sdf_field``, marching cubes against the numpy restatement tests/mesh_ref.py (exact), the geometry of the
extracted surfaces, and ``extract_geometry`` of the three drop-in models."""
import numpy as np
import pytest
import torch

import mesh_ref
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _fine_model(name="g16"):
    from esr_nerf_amd.config import fine_cfg
    from esr_nerf_amd.synthetic import init_slab_model, slab_scene
    from esr_nerf_amd.voxurff import VoxurfF
    sc = slab_scene(name)
    torch.manual_seed(0)
    m = VoxurfF(fine_cfg(DEV), sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max,
                sc.mask_alpha_init, sc.mask_density, sc.s_val, sc.num_voxels)
    return init_slab_model(m, sc)


@torch.no_grad()
def _sphere_grid(m, r=0.5, c=(0.1, -0.05, 0.0)):
    """|p - c| - r on the grid nodes of m (world space)."""
    ws = [int(v) for v in m.world_size]
    ax = [torch.linspace(float(m.xyz_min[a]), float(m.xyz_max[a]), ws[a], dtype=torch.float64) for a in range(3)]
    X, Y, Z = torch.meshgrid(*ax, indexing="ij")
    s = ((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2).sqrt() - r
    m.sdf.grid.copy_(s.float()[None, None].to(m.sdf.grid.device))
    return m


def _field_bound(m):
    return 2.0 ** -22 * float(m.sdf.grid.detach().abs().max())


@pytest.mark.parametrize("scene", ["slab", "sphere"])
@pytest.mark.parametrize("R", [2, 37, 64])
def test_field_unsmoothed_matches_torch(scene, R):
    from esr_nerf_amd.mesh import sdf_field
    from esr_nerf_amd.modules import extract_sdf_field
    m = _fine_model()
    if scene == "sphere":
        _sphere_grid(m)
    u = sdf_field(m, R, smooth=False)
    ref = extract_sdf_field(m, R, smooth=False)
    assert u.shape == ref.shape == (R, R, R) and u.is_cuda
    assert float((u - ref).abs().max()) <= _field_bound(m)


@pytest.mark.parametrize("scene", ["slab", "sphere"])
def test_field_smoothed_matches_torch(scene):
    from esr_nerf_amd.mesh import field, lattice_axes, sdf_field, smooth_grid
    from esr_nerf_amd.modules import Gaussian3DConv, extract_sdf_field
    m = _fine_model()
    if scene == "sphere":
        _sphere_grid(m)
    grid = m.sdf.grid.detach()
    with torch.no_grad():
        sm_torch = Gaussian3DConv(sigma=0.5).to(DEV)(grid)
    assert rel_err(smooth_grid(grid[0, 0].contiguous(), 0.5), sm_torch[0, 0]) < 1e-6
    lo, hi = m.xyz_min.float().cpu(), m.xyz_max.float().cpu()
    ref = extract_sdf_field(m, 45, smooth=True)
    u = field(sm_torch[0, 0].contiguous(), lo, hi, lattice_axes(lo, hi, 45, DEV))
    assert float((u - ref).abs().max()) <= _field_bound(m)
    # the whole HIP path (HIP smoothing): within the smoothing's own rounding of the torch path
    assert rel_err(sdf_field(m, 45, smooth=True), ref) < 4e-6


def _random_field(shape, seed, kind):
    g = torch.Generator().manual_seed(seed)
    if kind == "noise":
        return torch.randn(shape, generator=g)
    # smooth blobs + noise: a surface of moderate size at any R
    idx = [torch.linspace(0, 1, s, dtype=torch.float64) for s in shape]
    X, Y, Z = torch.meshgrid(*idx, indexing="ij")
    f = torch.zeros(shape, dtype=torch.float64)
    for _ in range(6):
        k = torch.rand(3, generator=g, dtype=torch.float64) * 12 + 2
        ph = torch.rand(3, generator=g, dtype=torch.float64) * 6.3
        f += torch.sin(k[0] * X + ph[0]) * torch.cos(k[1] * Y + ph[1]) * torch.sin(k[2] * Z + ph[2])
    return (f / 3 + 0.01 * torch.randn(shape, generator=g, dtype=torch.float64)).float()


def _check_exact(u, thr):
    from esr_nerf_amd.mesh import marching_cubes
    v, f = marching_cubes(u.to(DEV), thr)
    rv, rf = mesh_ref.marching_cubes(u.numpy(), thr)
    assert v.dtype == torch.float64 and f.dtype == torch.int64 and v.is_cuda and f.is_cuda
    assert v.shape == rv.shape and f.shape == rf.shape
    assert np.array_equal(v.cpu().numpy(), rv) and np.array_equal(f.cpu().numpy(), rf)
    return rv, rf


@pytest.mark.parametrize("shape,kind", [((17, 17, 17), "noise"), ((64, 40, 33), "noise"), ((64, 40, 33), "blobs"),
                                        ((256, 256, 256), "blobs")])
@pytest.mark.parametrize("thr", [0.0, 0.3])
def test_marching_cubes_equals_reference(shape, kind, thr):
    u = _random_field(shape, sum(shape), kind)
    v, f = _check_exact(u, thr)
    assert len(f) > 0


def test_marching_cubes_threshold_ties_and_empty():
    u = _random_field((19, 23, 21), 5, "noise")
    thr = 0.25
    u[:, 7, :] = thr                                  # a whole plane exactly at the threshold (outside)
    u[3, 4, 5] = thr
    u[11, 12, 13] = thr
    u[:, :, 20] = thr
    _check_exact(u, thr)
    u2 = _random_field((19, 23, 21), 6, "noise")
    u2[5:9] = 0.0                                      # thr 0: slabs of exact zeros
    _check_exact(u2, 0.0)
    from esr_nerf_amd.mesh import marching_cubes
    for field, t in ((torch.ones(9, 8, 7), 0.0), (-torch.ones(9, 8, 7), 0.0), (torch.full((6, 6, 6), 0.5), 0.5),
                     (torch.ones(2, 2, 2), 0.0)):
        v, f = marching_cubes(field.to(DEV), t)
        assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == torch.float64 and f.dtype == torch.int64
    _check_exact(torch.tensor([[[1.0, -1.0], [-1.0, 1.0]], [[-1.0, 1.0], [1.0, -1.0]]]), 0.0)   # R = 2, one cell


def _census(f):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key, inv, cnt = np.unique(np.sort(e, 1), axis=0, return_inverse=True, return_counts=True)
    bal = np.zeros(len(key), np.int64)
    np.add.at(bal, inv.reshape(-1), np.where(e[:, 0] < e[:, 1], 1, -1))
    return key, cnt, bal


def _lattice_u(R, fn):
    g = torch.arange(R, dtype=torch.float64, device=DEV)
    X, Y, Z = torch.meshgrid(g, g, g, indexing="ij")
    return fn(X, Y, Z).float().contiguous()


def _on_lattice_edges(v, R):
    frac = v - np.floor(v)
    assert ((frac != 0).sum(1) <= 1).all()
    assert (v >= 0).all() and (v <= R - 1).all()


def test_sphere_and_torus_geometry():
    from esr_nerf_amd.mesh import marching_cubes
    R, r = 128, 40.0
    c = (R - 1) / 2 + 0.3
    u = _lattice_u(R, lambda X, Y, Z: r - ((X - c) ** 2 + (Y - c) ** 2 + (Z - c) ** 2).sqrt())
    v, f = (t.cpu().numpy() for t in marching_cubes(u, 0.0))
    key, cnt, bal = _census(f)
    assert (cnt == 2).all() and (bal == 0).all()              # closed, every edge traversed once each way
    assert len(v) - len(key) + len(f) == 2
    vol = np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6
    assert vol > 0 and abs(vol / (4 / 3 * np.pi * r ** 3) - 1) < 0.01
    _on_lattice_edges(v, R)
    # a torus: Euler characteristic 0
    Rt, rt = 30.0, 12.0
    u = _lattice_u(R, lambda X, Y, Z: rt - ((((X - c) ** 2 + (Y - c) ** 2).sqrt() - Rt) ** 2 + (Z - c) ** 2).sqrt())
    v, f = (t.cpu().numpy() for t in marching_cubes(u, 0.0))
    key, cnt, bal = _census(f)
    assert (cnt == 2).all() and (bal == 0).all()
    assert len(v) - len(key) + len(f) == 0


def test_surface_meeting_the_box_is_open_only_on_lattice_faces():
    from esr_nerf_amd.mesh import marching_cubes
    R = 64
    u = _lattice_u(R, lambda X, Y, Z: 50.0 - (X ** 2 + Y ** 2 + (Z - 20) ** 2).sqrt())   # a ball cut by three faces
    v, f = (t.cpu().numpy() for t in marching_cubes(u, 0.0))
    key, cnt, bal = _census(f)
    open_ = (cnt != 2) | (bal != 0)
    assert open_.sum() > 100 and (cnt[open_] == 1).all()
    a, b = v[key[open_, 0]], v[key[open_, 1]]
    face = lambda p: (p == 0) | (p == R - 1)                                             # noqa: E731
    assert (face(a) & face(b)).any(1).all()


def _build(kind):
    from esr_nerf_amd.synthetic import analytic_sdf, slab_scene
    sc = slab_scene("C2g256")
    torch.manual_seed(0)
    np.random.seed(0)
    if kind == "VoxurfC":
        from esr_nerf_amd.config import coarse_cfg
        from esr_nerf_amd.voxurfc import VoxurfC
        m = VoxurfC(coarse_cfg(DEV, num_voxels=sc.num_voxels), sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min,
                    sc.mask_xyz_max, sc.mask_alpha_init, sc.mask_density, sc.s_val)
    elif kind == "VoxurfF":
        from esr_nerf_amd.config import fine_cfg
        from esr_nerf_amd.voxurff import VoxurfF
        m = VoxurfF(fine_cfg(DEV), sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max,
                    sc.mask_alpha_init, sc.mask_density, sc.s_val, sc.num_voxels)
    else:
        from esr_nerf_amd.config import lts_cfg
        from esr_nerf_amd.esrnerf import ESRNeRF
        m = ESRNeRF(lts_cfg(DEV), sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max,
                    sc.mask_alpha_init, sc.mask_density, sc.s_val, sc.num_voxels)
    ws = [int(v) for v in m.world_size]
    assert ws == [256, 256, 256]
    with torch.no_grad():
        m.sdf.grid.copy_(analytic_sdf(ws, sc.xyz_min, sc.xyz_max).to(DEV))
    return m


def _check_mesh(m, v, f, u, thr):
    lo, hi = m.xyz_min.float().cpu().numpy(), m.xyz_max.float().cpu().numpy()
    assert isinstance(v, np.ndarray) and isinstance(f, np.ndarray)
    assert v.dtype == np.float64 and f.dtype == np.int64 and v.ndim == 2 and v.shape[1] == 3 and f.shape[1] == 3
    assert len(f) > 0 and (v >= lo).all() and (v <= hi).all() and f.min() >= 0 and f.max() < len(v)
    assert (len(v), len(f)) == mesh_ref.counts(u.cpu().numpy(), thr)


@pytest.mark.parametrize("kind", ["VoxurfF", "ESRNeRF", "VoxurfC"])
def test_extract_geometry_of_the_drop_in_models(kind):
    from esr_nerf_amd.mesh import sdf_field
    m = _build(kind)
    v, f = m.extract_geometry()                                   # the trainers' call: R = 512, smoothed
    _check_mesh(m, v, f, sdf_field(m, 512), 0.0)
    if kind != "VoxurfF":
        return
    v2, f2 = m.extract_geometry()
    assert v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes()            # byte-identical run to run
    v, f = m.extract_geometry(resolution=None, threshold=0.05, smooth=False, batch_size=7)
    _check_mesh(m, v, f, sdf_field(m, 256, smooth=False), 0.05)
    v, f = m.extract_geometry(resolution=100, threshold=-0.1)
    _check_mesh(m, v, f, sdf_field(m, 100), -0.1)


def test_runs_are_byte_identical():
    from esr_nerf_amd.mesh import marching_cubes
    u = _random_field((96, 80, 72), 3, "noise").to(DEV)
    a = [t.cpu().numpy().tobytes() for t in marching_cubes(u, 0.1)]
    b = [t.cpu().numpy().tobytes() for t in marching_cubes(u, 0.1)]
    assert a == b
