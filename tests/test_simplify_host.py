"""mesh.simplify's restatement (tests/simplify_ref.py) checked without a GPU: the exact form against a brute force that
takes the definition word by word in ``fractions.Fraction``; the properties the definition promises, in exact arithmetic;
the float64 numpy form and the emulation of the kernel's order inside every bound the GPU is held to; mutants of the
definition, each rejected; the C header against the ctypes signatures; the entry points' argument checks; no scratch."""
import ctypes
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import simplify_ref as sr
from conftest import ROOT

ENTRIES = ("esr_simplify_cell_keys", "esr_simplify_pair_keys", "esr_simplify_clusters", "esr_simplify_face_keys",
           "esr_simplify_keep")
KERNELS = ("simplify_cell_keys_kernel", "simplify_pair_keys_kernel", "simplify_cluster_lane_kernel", "simplify_cluster_group_kernel", "simplify_face_keys_kernel",
           "simplify_keep_kernel")
_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def case(name):
    """-> (v, t, h, attr)"""
    def make():
        if name == "sphere":
            v, t = sr.uv_sphere(10, 14)
            return v * 0.9 + 0.03, t, 0.45, sr.attributes(v, 5)
        if name == "cube":
            v, t = sr.cube(5)
            return v + 0.013, t, 0.37, sr.attributes(v, 3, seed=1)
        v, t, h = sr.edge_case(name)
        return v, t, h, sr.attributes(v, 4, seed=2)
    return memo(("case", name), make)


def exact_of(name):
    return memo(("exact", name), lambda: sr.exact(*case(name)[:3], 1e-3, case(name)[3]))


SMALL = ("sphere", "cube") + sr.EDGE_CASES


def test_longdouble_is_the_x87_format():
    assert np.finfo(np.longdouble).eps == 2.0 ** -63


# ---- brute force: the definition word by word, every face tried against every cluster


def brute(v, t, h, lam):
    o = v.min(0)
    cells = [tuple(int(math.floor((v[i, a] - o[a]) / h)) for a in range(3)) for i in range(len(v))]
    order = sorted(set(cells))
    out = []
    for c in order:
        g = [float(np.float64(o[a]) + np.float64(c[a] + 0.5) * np.float64(h)) for a in range(3)]
        rel = lambda i: [Fraction(float(np.float64(v[i, a]) - np.float64(g[a]))) for a in range(3)]      # noqa: E731
        mem = [i for i in range(len(v)) if cells[i] == c]
        hh = Fraction(float(h)) / 2
        xbar = [min(max(sum(rel(i)[a] for i in mem) / len(mem), -hh), hh) for a in range(3)]
        A, b, cc, S = [Fraction(0)] * 6, [Fraction(0)] * 3, Fraction(0), Fraction(0)
        for tri in t:
            if not any(cells[i] == c for i in tri):
                continue
            p0, p1, p2 = (rel(i) for i in tri)
            e1, e2 = [p1[a] - p0[a] for a in range(3)], [p2[a] - p0[a] for a in range(3)]
            n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            d = -sum(n[a] * p0[a] for a in range(3))
            A = [A[q] + n[i] * n[j] for q, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)))]
            b = [b[a] + n[a] * d for a in range(3)]
            cc += d * d
            S += sum(x * x for x in e1) * sum(x * x for x in e2)
        out.append((A + b + [cc, S], xbar, sr.solve_clip(A, b, S, xbar, h, lam)))
    return order, cells, out


def brute_faces(cluster_of, t):
    kept = []
    for f, tri in enumerate(t):
        ks = [cluster_of[i] for i in tri]
        if ks[0] == ks[1] or ks[0] == ks[2] or ks[1] == ks[2]:
            continue
        if any(set(ks) == set(cluster_of[i] for i in t[e]) for e in kept):
            continue
        kept.append(f)
    named = sorted({cluster_of[i] for f in kept for i in t[f]})
    return [[named.index(cluster_of[i]) for i in t[f]] for f in kept], kept, named


@pytest.mark.parametrize("name", sr.EDGE_CASES + ("cube",))
def test_exact_form_equals_the_brute_force(name):
    v, t, h, _ = case(name)
    if name == "cube":
        v, t = sr.cube(2)
        v, h = v + 0.013, 0.6
        ex = sr.exact(v, t, h, 1e-3)
    else:
        ex = exact_of(name)
    order, cells, out = brute(v, t, h, 1e-3)
    assert [(int(k >> 42), int(k >> 21) & 0x1fffff, int(k) & 0x1fffff) for k in ex.keys] == order
    assert [order.index(c) for c in cells] == ex.vc.tolist()
    for k, (sums, xbar, y) in enumerate(out):
        assert sums == ex.sums[k][:11] and xbar == ex.xbar[k] and y == ex.y[k], k
    tri, origin, new_id = sr.faces(ex.vc, t, len(order))
    btri, bkept, named = brute_faces(ex.vc.tolist(), t.tolist())
    assert tri.tolist() == btri and origin.tolist() == bkept
    assert [k for k in range(len(order)) if new_id[k] >= 0] == named


def test_the_edge_cases_are_what_their_names_say():
    ex = exact_of("collinear_and_coincident")
    v, t, h, _ = case("collinear_and_coincident")
    assert len({ex.vc[i] for i in (5, 6, 7)}) == 1 and np.array_equal(v[2], v[8])
    # face 2: the cross product of the float64 inputs r = fl(v - g) is exactly 0 and s is positive; face 3: s is 0
    r = [[Fraction(float(x)) for x in v[i] - ex.g[ex.vc[5]]] for i in (5, 6, 7)]
    assert all(Fraction(float(v[i][a])) - Fraction(float(ex.g[ex.vc[5]][a])) == r[j][a] for j, i in enumerate((5, 6, 7)) for a in range(3))
    e1, e2 = [r[1][a] - r[0][a] for a in range(3)], [r[2][a] - r[0][a] for a in range(3)]
    assert [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]] == [0, 0, 0]
    assert sum(x * x for x in e1) * sum(x * x for x in e2) > 0
    assert sum((Fraction(float(v[8][a])) - Fraction(float(v[2][a]))) ** 2 for a in range(3)) == 0
    ex = exact_of("all_degenerate_cluster")
    k = ex.vc[3]
    assert ex.vc[4] == k and ex.sums[k][10] == 0 and ex.sums[k][11] == 0 and ex.fallback[k] and ex.y[k] == ex.xbar[k]
    assert ex.attr[k] == [Fraction(float(a)) for a in case("all_degenerate_cluster")[3][3]]
    v, t, h, _ = case("two_sheets")
    tri, origin, _ = sr.faces(exact_of("two_sheets").vc, t, 4)
    assert origin.tolist() == [0, 3] and tri.tolist() == [[0, 2, 1], [2, 3, 1]]
    v, t, h, _ = case("on_cell_borders")
    on = (v - v.min(0)) / h
    assert np.array_equal(2 * on, np.round(2 * on)) and (on == np.round(on)).any(1).all() and on.max() == 2.0
    for name in ("one_cell", "no_faces"):
        ex = exact_of(name)
        tri, origin, new_id = sr.faces(ex.vc, case(name)[1], len(ex.keys))
        assert len(tri) == 0 and (new_id == -1).all()
    assert len(exact_of("one_cell").keys) == 1


@pytest.mark.parametrize("name", SMALL)
def test_new_vertices_stay_in_their_cells_and_never_raise_the_quadric_error(name):
    ex = exact_of(name)
    hh = Fraction(ex.h) / 2
    moved = 0
    for k in range(len(ex.sums)):
        A, b, c = ex.sums[k][:6], ex.sums[k][6:9], ex.sums[k][9]
        assert all(-hh <= y <= hh for y in ex.y[k]) and all(-hh <= x <= hh for x in ex.xbar[k])
        assert sr.quadric_error(A, b, c, ex.y[k]) <= sr.quadric_error(A, b, c, ex.xbar[k])
        # tr A <= S: the matrix of the solve is SPD with condition number <= 1 + 1 / lam
        assert A[0] + A[3] + A[5] <= ex.sums[k][10]
        moved += ex.y[k] != ex.xbar[k]
    assert moved or name in ("no_faces", "all_degenerate_cluster")


def result_rows(res, ex):
    return dict(sums=res["sums"], xbar=res["xbar"], pos=res["pos"], attr=res["attr"])


@pytest.mark.parametrize("name", SMALL)
def test_float64_form_and_kernel_order_sit_inside_the_gpu_bounds(name):
    v, t, h, attr = case(name)
    ex = exact_of(name)
    for what, big, res in (("fast", None, sr.fast(v, t, h, 1e-3, attr)), ("default", sr.BIG, sr.emulate(v, t, h, 1e-3, attr, big=sr.BIG)),
                           ("serial", 1 << 20, sr.emulate(v, t, h, 1e-3, attr, big=1 << 20)),
                           ("tree", 4, sr.emulate(v, t, h, 1e-3, attr, big=4))):
        assert np.array_equal(res["keys"], ex.keys) and np.array_equal(res["vc"], ex.vc)
        worst, fails = sr.check(ex, result_rows(res, ex), what, big)
        print(f"  {name:26s} {what:7s} " + " ".join(f"{k} {x:.3f}" for k, x in worst.items()))
        assert not fails, fails[:5]


def test_kernel_order_on_a_large_cluster_sits_inside_the_gpu_bounds():
    """one cluster of 1 682 faces on 900 vertices: the strided partial sums make seven trips, then the fold"""
    assert sr.BIG < 900
    v, t = sr.dense_patch(30)
    attr = sr.attributes(v, 3, seed=5)
    ex = sr.exact(v, t, 1.0, 1e-3, attr)
    assert len(ex.keys) == 1
    for what, big in (("tree", sr.BIG), ("serial", 1 << 20)):
        worst, fails = sr.check(ex, sr.emulate(v, t, 1.0, 1e-3, attr, big=big), what, big)
        print(f"  dense_patch(30) {what:7s} " + " ".join(f"{k} {x:.3f}" for k, x in worst.items()))
        assert not fails, fails[:5]


MUTANT_CASE = {"per_corner": "sphere", "unit_normal": "sphere", "trace_regulariser": "collinear_and_coincident",
               "projection_clamp": "sphere", "centre_pull": "sphere", "unweighted_attr": "sphere"}
FACE_MUTANT_CASE = {"keep_degenerate": "sphere", "keep_duplicates": "two_sheets", "keep_later": "two_sheets",
                    "normalise_winding": "two_sheets", "keep_unreferenced": "all_degenerate_cluster"}


@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_every_mutant_of_the_sums_and_the_position_is_rejected(mutant):
    name = MUTANT_CASE[mutant]
    v, t, h, attr = case(name)
    ex = exact_of(name)
    _, fails = sr.check(ex, result_rows(sr.fast(v, t, h, 1e-3, attr, mutant=mutant), ex), mutant, None)
    assert fails
    if mutant == "trace_regulariser":                               # ... in the cluster that holds the collinear face
        assert any(f" cluster {ex.vc[5]} position" in f for f in fails), fails
    if mutant == "per_corner":                                      # a face with two corners in a cluster was counted twice
        inc = sr.incident(ex.vc, t, mutant)
        assert any(len(fs) != len(set(fs)) for fs in inc)


@pytest.mark.parametrize("mutant", sr.FACE_MUTANTS)
def test_every_mutant_of_the_face_rules_is_rejected(mutant):
    name = FACE_MUTANT_CASE[mutant]
    t = case(name)[1]
    ex = exact_of(name)
    good, bad = sr.faces(ex.vc, t, len(ex.keys)), sr.faces(ex.vc, t, len(ex.keys), mutant=mutant)
    assert any(a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(good, bad))


def test_grid_refuses_what_the_definition_refuses():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    for bad_h in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError):
            sr.grid(v, bad_h)
    with pytest.raises(ValueError):
        sr.grid(np.array([[0.0, math.nan, 0.0]]), 1.0)
    with pytest.raises(ValueError):
        sr.grid(v * (2 ** 21 - 1), 1.0)                             # cells 0 .. 2^21 - 1: one too many
    assert len(sr.grid(v * (2 ** 21 - 2), 1.0)[1]) == 2             # cells 0 .. 2^21 - 2


# ---- the library: header, signatures, argument checks, generated code


def test_header_declares_the_simplify_entry_points_and_ctypes_agrees():
    from esr_nerf_amd import _lib, mesh
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    # the names only: tests/test_host.py checks every entry's restype and argument types against the header text
    for name in ENTRIES:
        assert name in _lib.EXPORTS and _lib.SIGNATURES[name][0] is ctypes.c_int, name
    assert int(re.search(r"#define ESR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == _lib.lib().esr_abi_version()
    assert int(re.search(r"#define ESR_SIMPLIFY_MAX_C (\d+)", header).group(1)) == _lib.SIMPLIFY_MAX_C == 16
    assert int(re.search(r"#define ESR_SIMPLIFY_DEBUG (\d+)", header).group(1)) == _lib.SIMPLIFY_DEBUG == 15
    assert mesh.SIMPLIFY_MAX_CELLS == sr.MAX_CELLS and mesh.SIMPLIFY_BIG == sr.BIG and mesh.SIMPLIFY_TRIALS == 24


def test_entry_points_check_their_arguments_before_any_launch():
    """Every code here is returned by the host-side checks: no pointer is read and nothing is launched"""
    from esr_nerf_amd import _lib
    L = _lib.lib()
    null, p, odd = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    odd2 = ctypes.c_void_p(0x1002)

    def keys(v=p, nv=5, o=p, h=0.5, out=p):
        return L.esr_simplify_cell_keys(v, nv, o, h, out, null)

    for kw in (dict(nv=-1), dict(h=0.0), dict(h=-1.0), dict(h=math.nan), dict(h=math.inf), dict(v=null), dict(o=null),
               dict(out=null), dict(v=odd), dict(o=odd), dict(out=odd)):
        assert keys(**kw) == -1, kw
    assert keys(nv=1 << 31) == -2 and keys(nv=0, v=null, o=null, out=null) == 0

    def pairs(t=p, nf=4, vc=p, nv=5, out=p):
        return L.esr_simplify_pair_keys(t, nf, vc, nv, out, null)

    for kw in (dict(nf=-1), dict(nv=-1), dict(t=null), dict(vc=null), dict(out=null), dict(t=odd), dict(vc=odd2), dict(out=odd)):
        assert pairs(**kw) == -1, kw
    assert pairs(nf=1 << 31) == -2 and pairs(nv=1 << 31) == -2 and pairs(nf=0, t=null, vc=null, out=null) == 0

    def clusters(v=p, nv=5, t=p, nf=4, vc=p, ck=p, nk=3, ms=p, mi=p, ps=p, pr=p, npairs=12, o=p, h=0.5, lam=1e-3, attr=p, nc=2,
                 big=64, pos=p, ao=p, dbg=null):
        return L.esr_simplify_clusters(v, nv, t, nf, vc, ck, nk, ms, mi, ps, pr, npairs, o, h, lam, attr, nc, big, pos, ao, dbg, null)

    for kw in (dict(nv=-1), dict(nf=-1), dict(nk=-1), dict(npairs=-1), dict(nc=-1), dict(big=0), dict(h=0.0), dict(h=math.nan),
               dict(lam=0.0), dict(lam=math.inf), dict(lam=math.nan), dict(npairs=13), dict(nk=6), dict(v=null), dict(vc=null),
               dict(ck=null), dict(ms=null), dict(mi=null), dict(ps=null), dict(o=null), dict(pos=null), dict(t=null),
               dict(pr=null), dict(attr=null), dict(ao=null), dict(v=odd), dict(pos=odd), dict(dbg=odd), dict(pr=odd),
               dict(vc=odd2), dict(attr=odd2), dict(ao=odd2)):
        assert clusters(**kw) == -1, kw
    for kw in (dict(nc=17), dict(nv=1 << 31), dict(nf=1 << 31, npairs=0)):
        assert clusters(**kw) == -2, kw
    assert clusters(nk=0, v=null, pos=null) == 0

    def fkeys(t=p, nf=4, vc=p, nv=5, hi=p, lo=p):
        return L.esr_simplify_face_keys(t, nf, vc, nv, hi, lo, null)

    for kw in (dict(nf=-1), dict(nv=-1), dict(t=null), dict(vc=null), dict(hi=null), dict(lo=null), dict(hi=odd), dict(lo=odd2)):
        assert fkeys(**kw) == -1, kw
    assert fkeys(nf=1 << 31) == -2 and fkeys(nf=0, t=null, hi=null, lo=null) == 0

    def keep(order=p, hi=p, lo=p, nf=4, t=p, vc=p, nv=5, nk=3, out=p, used=p):
        return L.esr_simplify_keep(order, hi, lo, nf, t, vc, nv, nk, out, used, null)

    for kw in (dict(nf=-1), dict(nv=-1), dict(nk=-1), dict(nk=6), dict(order=null), dict(hi=null), dict(lo=null), dict(t=null),
               dict(vc=null), dict(out=null), dict(used=null), dict(order=odd), dict(lo=odd2)):
        assert keep(**kw) == -1, kw
    assert keep(nf=1 << 31) == -2 and keep(nf=0, nk=0, order=null, hi=null, lo=null, t=null, out=null, used=null) == 0


def test_python_layer_refuses_before_any_launch():
    from esr_nerf_amd import mesh, sources
    v, t = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.int64)
    for fn in (lambda: mesh.simplify(v, t, 0.5), lambda: mesh.simplify_to(v, t, 10)):                 # CPU tensors
        with pytest.raises(ValueError, match="device tensor"):
            fn()
    surf = sources.Surface(v, t, {})
    for kw in (dict(), dict(cell=0.5, target_faces=10)):
        with pytest.raises(ValueError, match="exactly one"):
            sources.simplify_surface(surf, **kw)
    with pytest.raises(ValueError, match="face_source"):
        sources.simplify_surface(surf, cell=0.5, face_source=torch.zeros(3, dtype=torch.int32))
    assert "simplify_surface" in sources.__all__


def test_simplify_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta as km
    meta = km.kernel_meta(km.asm_of(os.path.join(ROOT, "esr_nerf_amd", "csrc", "simplify.hip")))
    assert len(meta) == len(KERNELS), list(meta)
    for name in KERNELS:
        ks = [v for k, v in meta.items() if name in k]
        assert len(ks) == 1, (name, list(meta))
        assert ks[0].get("scratch", 0) == 0 and ks[0].get("spill_v", 0) == 0, (name, ks[0])
