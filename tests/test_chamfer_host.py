"""The DTU Chamfer metric's CPU side: the numpy restatement tests/chamfer_ref.py against the reference's own DTU_CD
(tests/golden/dtu_cd_small.npz, tools/gen_dtu_cd_golden.py) and against sklearn's radius_neighbors loop, and the file
readers of esr_nerf_amd/chamfer.py (PLY, the DTU .mat files)."""
import numpy as np
import pytest

import chamfer_ref
from conftest import load_npz
from esr_nerf_amd import chamfer


def test_restatement_matches_the_reference_golden():
    z = load_npz("dtu_cd_small.npz")
    got = chamfer_ref.dtu_cd(z["vertices"], z["triangles"], z["obs_mask"], z["bb"], z["res"], z["stl"], z["plane"],
                             z["perm"], float(z["max_dist"]), int(z["patch"]), float(z["thresh"]))
    for g, k in zip(got, ("mean_d2s", "mean_s2d", "overall")):
        assert g == pytest.approx(float(z[k]), rel=1e-12, abs=0), k


def _cloud(n, seed):
    """random points with exact duplicates and pairs at exactly 0.25 (a power of two: the boundary is representable)"""
    rng = np.random.default_rng(seed)
    p = np.round(rng.uniform(0, 4, (n, 3)) * 64) / 64
    p[n // 2:n // 2 + 20] = p[:20]                               # duplicates
    p[n // 2 + 20:n // 2 + 40] = p[20:40] + np.array([0.25, 0, 0])  # exactly thresh away along x
    return p


def test_restatement_downsample_matches_sklearn_radius_loop():
    skln = pytest.importorskip("sklearn.neighbors")
    thresh = 0.25
    for seed in range(3):
        p = _cloud(3000, seed)
        order = np.random.default_rng(100 + seed).permutation(len(p)) if seed else np.arange(len(p))
        data = p[order]
        idxs = skln.NearestNeighbors(radius=thresh, algorithm="kd_tree").fit(data).radius_neighbors(
            data, radius=thresh, return_distance=False)
        mask = np.ones(len(data), bool)
        for cur, ids in enumerate(idxs):
            if mask[cur]:
                mask[ids] = 0
                mask[cur] = 1
        keep = chamfer_ref.downsample(data, thresh)
        assert np.array_equal(keep, mask)
        assert 0 < keep.sum() < len(p)


def _ply_header(fmt, n, props, faces=0):
    h = ["ply", f"format {fmt} 1.0", "comment extra properties", f"element vertex {n}"]
    h += [f"property {t} {name}" for name, t in props]
    if faces:
        h += [f"element face {faces}", "property list uchar int vertex_indices"]
    return "\n".join(h + ["end_header"]) + "\n"


def test_ply_round_trip_binary_and_ascii(tmp_path):
    rng = np.random.default_rng(0)
    v = rng.standard_normal((57, 3)) * 100
    f = rng.integers(0, 57, (31, 3))
    path = str(tmp_path / "mesh.ply")
    chamfer.write_ply(path, v, f)
    rv, rf = chamfer.read_ply(path)
    assert rv.dtype == np.float64 and np.array_equal(rv, v) and np.array_equal(rf, f)
    chamfer.write_ply(path, v)
    rv, rf = chamfer.read_ply(path)
    assert np.array_equal(rv, v) and rf is None

    # binary little-endian with extra float / uchar vertex properties around float32 x, y, z (the DTU stl layout)
    props = [("nx", "float"), ("x", "float"), ("y", "float"), ("red", "uchar"), ("z", "float"), ("value", "double")]
    dt = np.dtype([("nx", "<f4"), ("x", "<f4"), ("y", "<f4"), ("red", "u1"), ("z", "<f4"), ("value", "<f8")])
    rec = np.zeros(57, dt)
    v32 = v.astype(np.float32)
    rec["x"], rec["y"], rec["z"], rec["nx"], rec["red"], rec["value"] = v32[:, 0], v32[:, 1], v32[:, 2], 1.5, 7, -2.0
    with open(path, "wb") as fh:
        fh.write(_ply_header("binary_little_endian", 57, props).encode())
        fh.write(rec.tobytes())
    rv, rf = chamfer.read_ply(path)
    assert np.array_equal(rv, v32.astype(np.float64)) and rf is None

    # ASCII with extra properties and a face list
    lines = [f"{i} {float(x)!r} 3 {float(y)!r} {float(z)!r}" for i, (x, y, z) in enumerate(v)]
    with open(path, "w") as fh:
        fh.write(_ply_header("ascii", 57, [("id", "int"), ("x", "double"), ("flag", "uchar"), ("y", "double"),
                                           ("z", "double")], faces=len(f)))
        fh.write("\n".join(lines) + "\n")
        fh.write("\n".join(f"3 {a} {b} {c}" for a, b, c in f) + "\n")
    rv, rf = chamfer.read_ply(path)
    assert np.array_equal(rv, v) and np.array_equal(rf, f)


def test_load_dtu_pcd_reads_the_mat_files_and_the_stl_cloud(tmp_path):
    from scipy.io import savemat
    rng = np.random.default_rng(1)
    scene = 24
    (tmp_path / "ObsMask").mkdir()
    (tmp_path / "Points" / "stl").mkdir(parents=True)
    obs = rng.random((5, 6, 7)) > 0.5
    bb = np.array([[-10.5, -3.25, 1.0], [20.0, 30.125, 40.0]])
    savemat(str(tmp_path / "ObsMask" / f"ObsMask{scene}_10.mat"), {"ObsMask": obs, "BB": bb, "Res": np.array([[0.2]])})
    plane = np.array([[0.1], [0.2], [0.97], [-5.0]])
    savemat(str(tmp_path / "ObsMask" / f"Plane{scene}.mat"), {"P": plane})
    stl = rng.standard_normal((100, 3))
    chamfer.write_ply(str(tmp_path / "Points" / "stl" / f"stl{scene:03}_total.ply"), stl)
    O, B, R, S, P = chamfer.load_dtu_pcd(str(tmp_path), scene)
    assert np.array_equal(O.astype(bool), obs) and O.shape == obs.shape
    assert np.array_equal(B, bb) and float(R.reshape(-1)[0]) == 0.2
    assert np.array_equal(S, stl) and np.array_equal(P, plane)
