"""Host checks of the surface export (no GPU): the restatement of the component contract (tests/surface_ref.py) against
scipy's connected components, five mutants of the contract that it must reject, the device-free mesh filter, the PLY
writer against chamfer.read_ply, and the regeneration of tests/golden/surface_points.npz from the reference."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import surface_ref as sr
from conftest import ROOT, load_npz


def _cases():
    v, t = sr.strip(301, 1)
    yield "strip", v, t, None
    v, t = sr.disjoint(40)
    yield "disjoint", v, t, None
    v, t, m = sr.sheet_with_floaters(9, 7)
    yield "sheet", v, t, m
    yield "sheet_unmasked", v, t, None
    rng = np.random.default_rng(3)
    t = rng.integers(0, 60, (45, 3))
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
    yield "soup", rng.random((60, 3)), t, (rng.random(len(t)) < 0.6).astype(np.uint8)


@pytest.mark.parametrize("name,v,t,m", list(_cases()), ids=[c[0] for c in _cases()])
def test_restatement_equals_scipy_on_the_vertex_graph(name, v, t, m):
    lab, k = sr.components(t, len(v), m)
    lab2, k2 = sr.components_scipy(t, len(v), m)
    assert k == k2 and np.array_equal(lab, lab2)
    assert ((lab == -1) == (np.zeros(len(t), bool) if m is None else m == 0)).all()
    expect = {"strip": 1, "disjoint": 40, "sheet": 6, "sheet_unmasked": 6}
    if name in expect:
        assert k == expect[name]


def test_hand_checked_small_cases():
    # two triangles that share one vertex: one component; with that vertex duplicated: two
    assert sr.components([[0, 1, 2], [2, 3, 4]], 5)[1] == 1
    lab, k = sr.components([[0, 1, 2], [5, 3, 4]], 6)
    assert k == 2 and lab.tolist() == [0, 1]
    # numbered by the smallest vertex id, not by face order
    lab, k = sr.components([[7, 8, 9], [0, 1, 2], [9, 10, 11]], 12)
    assert k == 2 and lab.tolist() == [1, 0, 1]
    assert sr.components(np.zeros((0, 3), np.int64), 4) [1] == 0
    # a right triangle with legs 3 and 4: area 6, centroid (1, 4/3, 0)
    st = sr.stats([[0, 0, 0], [3, 0, 0], [0, 4, 0]], [[0, 1, 2]], [0], 1, np.array([[1.0], [2.0], [6.0]], np.float32))
    assert st["area"][0] == 6.0 and np.allclose(st["centroid"][0], [1.0, 4.0 / 3.0, 0.0], rtol=1e-15)
    assert st["area_attr"][0, 0] == 18.0 and st["mean_attr"][0, 0] == 3.0 and st["peak"][0] == 6.0
    assert st["bbox_min"][0].tolist() == [0, 0, 0] and st["bbox_max"][0].tolist() == [3, 4, 0]


# each mutant changes the answer on a small case, so a kernel (or restatement) that implemented it would be caught
def test_mutant_edge_adjacency_is_rejected():
    t = [[0, 1, 2], [2, 3, 4]]                   # a bow tie: one shared vertex, no shared edge
    assert sr.components(t, 5)[1] == 1 and sr.components(t, 5, adjacency="edge")[1] == 2


def test_mutant_first_face_order_is_rejected():
    t = [[7, 8, 9], [0, 1, 2]]
    assert sr.components(t, 10)[0].tolist() == [1, 0]
    assert sr.components(t, 10, order="first_face")[0].tolist() == [0, 1]


def test_mutant_unselected_faces_that_link_is_rejected():
    t, m = [[0, 1, 2], [2, 3, 4], [4, 5, 6]], [1, 0, 1]
    lab, k = sr.components(t, 7, m)
    assert k == 2 and lab.tolist() == [0, -1, 1]
    lab, k = sr.components(t, 7, m, unselected_link=True)
    assert k == 1 and lab.tolist() == [0, -1, 0]


def test_mutant_area_without_the_half_is_rejected():
    v, t = [[0, 0, 0], [3, 0, 0], [0, 4, 0]], [[0, 1, 2]]
    assert sr.stats(v, t, [0], 1)["area"][0] == 6.0 and sr.stats(v, t, [0], 1, half=False)["area"][0] == 12.0


def test_mutant_unweighted_mean_is_rejected():
    v = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [10, 0, 0], [0, 10, 0]]
    t = [[0, 1, 2], [0, 3, 4]]                   # areas 0.5 and 50
    a = np.array([[0], [0], [0], [3], [3]], np.float32)      # face means 0 and 2
    good, bad = sr.stats(v, t, [0, 0], 1, a), sr.stats(v, t, [0, 0], 1, a, weighted=False)
    assert abs(good["mean_attr"][0, 0] - 100.0 / 50.5) < 1e-14 and abs(bad["mean_attr"][0, 0] - 1.0) < 1e-14


def test_sum_bound_holds_for_a_reordered_float64_sum():
    v, t = sr.strip(5000, 2)
    T = sr.face_terms(v, t)
    exact = sr.stats(v, t, np.zeros(len(t), np.int32), 1)
    for order in (np.arange(len(t)), np.arange(len(t))[::-1], np.random.default_rng(0).permutation(len(t))):
        s = 0.0
        for x in T["area"][order]:
            s += x
        assert abs(s - exact["area"][0]) <= sr.sum_bound(exact["n_faces"], exact["abs_area"])[0]


def test_keep_components_preserves_order_and_drops_unreferenced_vertices():
    from esr_nerf_amd import mesh
    v, t, m = sr.sheet_with_floaters(5, 4)
    lab, k = sr.components(t, len(v), m)
    keep = (lab == 1) | (lab == k - 1)
    v2, t2 = mesh.keep_components(torch.from_numpy(v), torch.from_numpy(t), torch.from_numpy(keep))
    used = np.unique(t[keep])
    assert np.array_equal(v2.numpy(), v[used])                                 # the referenced vertices in their order
    assert np.array_equal(used[t2.numpy()], t[keep])                           # the kept faces in their order
    v3, t3 = mesh.keep_components(torch.from_numpy(v), torch.from_numpy(t), torch.zeros(len(t), dtype=torch.bool))
    assert v3.shape == (0, 3) and t3.shape == (0, 3)
    with pytest.raises(ValueError):
        mesh.keep_components(torch.from_numpy(v), torch.from_numpy(t), torch.ones(3, dtype=torch.bool))


def _surface(n_v=23, n_f=31, seed=6):
    from esr_nerf_amd.sources import Surface
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    attrs = dict(normal=r(n_v, 3) - 0.5, sdf=r(n_v) - 0.5, basecolor=r(n_v, 3), roughness=r(n_v), metallic=r(n_v),
                 emission=r(n_v, 3) * 3)
    return Surface((torch.rand(n_v, 3, generator=g, dtype=torch.float64) - 0.5) * 1e3,
                   torch.randint(0, n_v, (n_f, 3), generator=g), attrs)


@pytest.mark.parametrize("with_source", [False, True])
def test_surface_ply_round_trip_and_header(tmp_path, with_source):
    from esr_nerf_amd.chamfer import _ply_header, read_ply
    from esr_nerf_amd.sources import VERTEX_PROPERTIES, write_surface_ply
    s = _surface()
    src = (torch.arange(s.triangles.shape[0], dtype=torch.int32) % 4) - 1
    path = str(tmp_path / "s.ply")
    write_surface_ply(path, s, src if with_source else None)
    v, f = read_ply(path)
    assert v.dtype == np.float64 and np.array_equal(v, s.vertices.numpy())     # bit for bit: double x y z
    assert f.dtype == np.int64 and np.array_equal(f, s.triangles.numpy())
    with open(path, "rb") as fh:
        fmt, elements = _ply_header(fh)
        body = fh.read()
    assert fmt == "binary_little_endian"
    (vn, vc, vprops), (fn, fc, fprops) = elements
    assert (vn, vc, fn, fc) == ("vertex", 23, "face", 31)
    assert [p for p, _ in vprops] == VERTEX_PROPERTIES
    assert [t for _, t in vprops] == ["double"] * 3 + ["float"] * 11
    assert fprops == [("vertex_indices", ("list", "uchar", "int"))] + ([("source", "int")] if with_source else [])
    assert len(body) == 23 * (24 + 44) + 31 * (13 + (4 if with_source else 0))
    vrec = np.frombuffer(body[:23 * 68], dtype=[(p, "<f8" if i < 3 else "<f4") for i, p in enumerate(VERTEX_PROPERTIES)])
    assert np.array_equal(np.stack([vrec["nx"], vrec["ny"], vrec["nz"]], 1), s.attrs["normal"].numpy())
    assert np.array_equal(vrec["roughness"], s.attrs["roughness"].numpy())
    assert np.array_equal(vrec["emission_b"], s.attrs["emission"][:, 2].numpy())
    if with_source:
        frec = np.frombuffer(body[23 * 68:], dtype=[("n", "u1"), ("v", "<i4", (3,)), ("source", "<i4")])
        assert np.array_equal(frec["source"], src.numpy())
        with pytest.raises(ValueError):
            write_surface_ply(path, s, src[:-1])


def test_surface_points_fixture_is_self_consistent():
    z = load_npz("surface_points.npz")
    assert z["points"].shape == (257, 3) and z["points"].dtype == np.float32
    for k, shape in dict(normal=(257, 3), sdf=(257,), basecolor=(257, 3), roughness=(257,), metallic=(257,),
                         emission=(257, 3)).items():
        assert z[k].shape == shape and z[k].dtype == np.float32 and np.isfinite(z[k]).all(), k
    k_val = float(z["k_val"].reshape(-1)[0])
    m = z["emission"].max(1)
    assert np.array_equal(z["emissive"], m > np.float32(k_val)) and 0 < z["emissive"].sum() < 257
    # no value within the parity bar (1e-4 max|emission| either way) of the threshold: no point needs an exemption
    assert np.abs(m.astype(np.float64) - k_val).min() >= 2e-4 * np.abs(z["emission"]).max() * (1 - 1e-6)


def test_surface_points_fixture_regenerates_bit_for_bit(tmp_path):
    """the generator in an interpreter of its own (other tests of a session leave stubs of the reference's packages in
    sys.modules), writing beside the committed file"""
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("the reference tree is not on this machine")
    env = dict(os.environ, ESR_GOLDEN_OUT=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_surface_golden.py")], env=env, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(str(tmp_path / "surface_points.npz")) as f:
        out = {k: f[k] for k in f.files}
    z = load_npz("surface_points.npz")
    assert set(out) == set(z)
    for k in z:
        assert out[k].dtype == z[k].dtype and np.array_equal(out[k], z[k]), k
