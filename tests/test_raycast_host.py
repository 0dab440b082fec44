"""The ray caster's restatement (tests/raycast_ref.py) checked without a GPU: the radix tree against an independent trie,
the boxes, a Python walk of the restated tree against the brute force on every case the GPU tests use, eight mutants of
that walk each rejected by the case it is listed for, the binary64 emulation of t inside its bound, the sample-point rule,
the C header against the ctypes signatures and the entry points' argument checks."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import raycast_ref as rr
from conftest import ROOT

ENTRIES = ("esr_bvh_keys", "esr_bvh_tree", "esr_bvh_fit", "esr_bvh_cast")
_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


MESHES = {"faces1": lambda: rr.few_faces(1), "faces2": lambda: rr.few_faces(2), "faces3": lambda: rr.few_faces(3),
          "lumpy": rr.lumpy_sphere, "twins": rr.twins, "chain": rr.chain, "nan_vertex": rr.with_nan_vertex,
          "far_small": rr.far_small, "room": lambda: rr.room()[:2]}


def mesh(name):
    return memo(("mesh", name), MESHES[name])


def built(name, nearest=False):
    return memo(("built", name, nearest), lambda: rr.built(*mesh(name), nearest=nearest))


def cases():
    def make():
        out = rr.sphere_cases("lumpy", *mesh("lumpy"))
        out.update(rr.other_cases(96))
        out.update(rr.room_cases())
        return out
    return memo("cases", make)


def case_ref(name):
    return memo(("ref", name), lambda: rr.case_brute(cases()[name]))


CASE_NAMES = ("lumpy/generic_cam", "lumpy/inside_cam", "lumpy/axis", "lumpy/special", "lumpy/interval", "lumpy/skip",
              "chain/random", "twins/random", "far_small/along_y", "nan_vertex/generic_cam", "faces1/random", "faces2/random",
              "faces3/random", "room/axis")


def test_the_case_list_is_complete():
    assert set(CASE_NAMES) == set(cases())


def test_longdouble_is_the_x87_format():
    assert np.finfo(np.longdouble).eps == 2.0 ** -63


# ---- the build


@pytest.mark.parametrize("name", sorted(MESHES))
def test_radix_tree_equals_the_trie_and_holds_every_face_once(name):
    T, nb, fb, k = built(name)
    n = len(k)
    ranges = rr.tree_ranges(T)
    assert set(ranges.values()) == rr.trie_tree(k) and len(ranges) == max(n - 1, 0)
    leaves = sorted(~int(c) for c in T.child.reshape(-1) if c < 0)
    assert leaves == list(range(n)) if n > 1 else leaves == []
    nodes = sorted(int(c) for c in T.child.reshape(-1) if c >= 0)
    assert nodes == list(range(1, n - 1)), "every node but the root is some node's child, once"
    for i in range(n - 1):                                          # the parent links are the child links read backwards
        for side in range(2):
            c = int(T.child[i, side])
            got = T.parent[c] if c >= 0 else T.leaf_parent[list(T.order).index(~c)]
            assert got == 2 * i + side
    if n > 1:
        assert T.parent[0] == -1
    # equal keys are told apart by their position: the order is stable
    assert all(k[a] < k[b] or (k[a] == k[b] and a < b) for a, b in zip(T.order[:-1], T.order[1:]))


def test_the_chain_is_deeper_than_64_levels_and_the_twins_share_one_key():
    assert built("chain")[0].depth > 64 and len(mesh("chain")[1]) == 80
    assert len(set(built("twins")[3].tolist())) == 1 and len(mesh("twins")[1]) == 1000
    k = built("nan_vertex")[3]
    bad = np.flatnonzero(~np.isfinite(mesh("nan_vertex")[0][mesh("nan_vertex")[1]]).all((1, 2)))
    assert len(bad) > 0 and (k[bad] == rr.KEY_NONE).all() and k.max() == rr.KEY_NONE
    assert np.isposinf(built("nan_vertex")[2][bad, :3]).all() and np.isneginf(built("nan_vertex")[2][bad, 3:]).all()


@pytest.mark.parametrize("name", sorted(MESHES))
def test_boxes_are_unions_and_hold_their_vertices_by_nextafter(name):
    v, tr = mesh(name)
    T, nb, fb, k = built(name)
    ok = np.isfinite(v[tr]).all((1, 2))
    lo, hi = v[tr].min(1), v[tr].max(1)
    f32 = np.float32
    for f in np.flatnonzero(ok):
        assert (fb[f, :3].astype(np.float64) <= lo[f]).all() and (fb[f, 3:].astype(np.float64) >= hi[f]).all()
        # ... and tight: one step inwards is inside the face's extent
        assert (np.nextafter(fb[f, :3], f32(np.inf)).astype(np.float64) > lo[f]).all()
        assert (np.nextafter(fb[f, 3:], f32(-np.inf)).astype(np.float64) < hi[f]).all()
    below = {}

    def faces_below(link):
        if link < 0:
            return [~link]
        if link not in below:
            below[link] = faces_below(int(T.child[link, 0])) + faces_below(int(T.child[link, 1]))
        return below[link]
    for i in range(len(T.child)):
        for side in range(2):
            c = int(T.child[i, side])
            fs = [f for f in faces_below(c) if ok[f]]
            if c >= 0:
                assert np.array_equal(nb[i, side, :3], np.minimum(nb[c, 0, :3], nb[c, 1, :3]))
                assert np.array_equal(nb[i, side, 3:], np.maximum(nb[c, 0, 3:], nb[c, 1, 3:]))
            if fs:
                assert (nb[i, side, :3].astype(np.float64) <= lo[fs].min(0)).all()
                assert (nb[i, side, 3:].astype(np.float64) >= hi[fs].max(0)).all()


# ---- the walk


def walk_case(name, mutant=None):
    c = cases()[name]
    mname = name.split("/")[0]
    T, nb, fb, k = built(mname, nearest=mutant == "nearest_boxes")
    n = len(c["o"])
    lo = np.broadcast_to(np.asarray(c.get("t_min", 0.0), np.float64), (n,))
    hi = np.broadcast_to(np.asarray(c.get("t_max", np.inf), np.float64), (n,))
    sk = c.get("skip", np.full(n, -1))
    got = [rr.walk(T, nb, c["v"], c["tr"], c["o"][i], c["d"][i], float(lo[i]), float(hi[i]), int(sk[i]), mutant=mutant)
           for i in range(n)]
    return np.array([g[0] for g in got], np.int64), np.array([g[1] for g in got])


def agrees(name, face, t, exact=False):
    """the walk's answer against the brute force: every unambiguous ray (or, `exact`, every ray: where the arithmetic of
    the two is the same, the rule decides every tie)"""
    ref = case_ref(name)
    sel = np.ones(len(face), bool) if exact else ~ref["ambiguous"]
    return np.array_equal(face[sel], ref["face"][sel]) and np.array_equal(t[sel], ref["t"][sel])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_python_walk_of_the_restated_tree_gives_the_brute_force_answer(name):
    face, t = walk_case(name)
    ref = case_ref(name)
    assert agrees(name, face, t)
    rr.check_hits(ref, face, t, np.zeros((len(face), 2)), name)
    if name == "twins/random":                                      # twin faces have the same t to the bit: the smaller id
        assert agrees(name, face, t, exact=True) and ref["ambiguous"].all() and (face[face >= 0] < 500).all()
    if cases()[name].get("generic"):
        assert ref["ambiguous"].mean() < 0.01
    print(f"  {name:26s} rays {len(face):5d} hit {int((face >= 0).sum()):5d} ambiguous {int(ref['ambiguous'].sum())}")


def t_min_exact_case():
    """t_min equal to the nearest hit's own t, to the bit: that face is NOT hit (t_min < t), the one behind it is"""
    c = dict(cases()["lumpy/skip"])
    base = rr.brute(c["v"], c["tr"], c["o"], c["d"])
    c.pop("skip")
    c["t_min"] = base["t"].copy()
    return c, base


MUTANT_CASE = {"exclusive_prune": "room/axis", "larger_id_on_ties": "twins/random", "t_min_inclusive": "t_min_exact",
               "cull_backfaces": "lumpy/inside_cam", "ignore_skip": "lumpy/skip", "nearest_boxes": "far_small/along_y",
               "zero_slab": "lumpy/axis", "no_eps": "segments"}


def segments_walk(mutant=None):
    v, tr, p, q, eps = rr.segment_case()
    T, nb, fb, k = built("lumpy")
    lo, hi = (0.0, 1.0) if mutant == "no_eps" else (eps, 1.0 - eps)
    got = np.array([rr.walk(T, nb, v, tr, p[i], q[i] - p[i], lo, hi, any_hit=True, mutant=mutant)[0] >= 0 for i in range(len(p))])
    ref = rr.brute(v, tr, p, q - p, eps, 1.0 - eps)
    assert not ref["ambiguous"].any() and not ref["hit"].any() and len(p) > 30
    return np.array_equal(got, ref["hit"])


def t_min_walk(mutant=None):
    c, base = t_min_exact_case()
    T, nb, fb, k = built("lumpy")
    face = np.array([rr.walk(T, nb, c["v"], c["tr"], c["o"][i], c["d"][i], float(c["t_min"][i]), mutant=mutant)[0]
                     for i in range(len(c["o"]))])
    ref = rr.brute(c["v"], c["tr"], c["o"], c["d"], c["t_min"])
    assert (ref["face"] != base["face"]).all() and (ref["t"][ref["face"] >= 0] > c["t_min"][ref["face"] >= 0]).all()
    return np.array_equal(face, ref["face"])


def holds(case, mutant=None):
    if case == "segments":
        return segments_walk(mutant)
    if case == "t_min_exact":
        return t_min_walk(mutant)
    return agrees(case, *walk_case(case, mutant), exact=case == "twins/random")


@pytest.mark.parametrize("mutant", rr.MUTANTS)
def test_every_mutant_of_the_walk_is_rejected_by_its_case(mutant):
    assert len(rr.MUTANTS) >= 8 and set(MUTANT_CASE) == set(rr.MUTANTS)
    case = MUTANT_CASE[mutant]
    assert holds(case), "the walk itself passes the case"
    assert not holds(case, mutant), (mutant, case)


# ---- t: the binary64 emulation inside the bound


@pytest.mark.parametrize("name", CASE_NAMES)
def test_emulated_t_sits_inside_the_bound(name):
    c, ref = cases()[name], case_ref(name)
    worst = rr.t_ratio(c["v"], c["tr"], c["o"], c["d"], ref)
    print(f"  {name:26s} worst |t - t_ref| / (2^-53 absref) = {worst:.3f}  (K_T = {rr.K_T}, recorded worst {rr.K_T_WORST})")
    assert worst <= rr.K_T
    assert rr.K_T_WORST <= rr.K_T < 2 * rr.K_T_WORST and math.log2(rr.K_T) == int(math.log2(rr.K_T))
    assert worst <= rr.K_T_WORST


# ---- source_visibility's sample points and the room


@pytest.mark.parametrize("samples", [1, 16, 100])
def test_sample_point_rule_against_a_direct_loop_and_the_room_is_unambiguous(samples):
    from esr_nerf_amd import sources
    v, tr, fs, S = rr.room()
    faces, points, margin = rr.source_samples(v, tr, fs, S, samples)
    assert margin > 1e-6, "no threshold within rounding of a cumulative area"
    surf = sources.Surface(torch.from_numpy(v), torch.from_numpy(tr), {})

    class Report:
        face_source = torch.from_numpy(fs)

        def __len__(self):
            return S
    face, point, n = sources.source_samples(surf, Report(), samples)
    assert face.shape == (S, samples) and point.shape == (S, samples, 3) and face.dtype == torch.int32
    for s in range(S):
        k = len(faces[s])
        assert int(n[s]) == k == min(samples, int((fs == s).sum()))
        assert np.array_equal(face[s, :k].numpy(), faces[s]) and np.array_equal(point[s, :k].numpy(), points[s])
    assert [int((fs == s).sum()) for s in range(S)] == [4, 4]
    share, bits, amb = rr.visibility(v, tr, fs, S, rr.room_points(), samples)
    assert amb == 0
    if samples == 16:
        # under the slab the ceiling patch is hidden; beside the slab part of it shows; behind another wall nothing does;
        # from behind its own wall a patch is seen whole (both windings count and the sample's own face is skipped)
        assert share[0, 0] == 0.0 and 0.0 < share[2, 0] <= 1.0 and (share[5] == 0.0).all() and share[4, 1] == 1.0
        assert share[6, 0] == 1.0 and share[7, 1] == 1.0
        print("  room shares\n", share)


def test_python_layer_refuses_before_any_launch():
    from esr_nerf_amd import raycast, sources
    v, t = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="device tensor"):
        raycast.build(v, t)
    assert "source_visibility" in sources.__all__ and "build" in raycast.__all__


# ---- the library: header, signatures, argument checks


def test_header_declares_the_bvh_entry_points_and_ctypes_agrees():
    from esr_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    # the names only: tests/test_host.py checks every entry's restype and argument types against the header text
    for name in ENTRIES:
        assert name in _lib.EXPORTS and _lib.SIGNATURES[name][0] is ctypes.c_int, name
    assert int(re.search(r"#define ESR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == _lib.lib().esr_abi_version()
    assert re.search(r"float box\[2\]\[6\];\s*int32_t child\[2\];\s*int32_t parent;\s*int32_t pad;", header)
    from esr_nerf_amd import raycast
    assert raycast.NODE_WORDS * 4 == 64


def test_entry_points_check_their_arguments_before_any_launch():
    """Every code here is returned by the host-side checks: no pointer is read and nothing is launched"""
    from esr_nerf_amd import _lib
    L = _lib.lib()
    null, p, odd = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    odd2, odd8 = ctypes.c_void_p(0x1002), ctypes.c_void_p(0x1008)
    big = 1 << 31

    def keys(v=p, nv=5, t=p, nf=4, sb=p, k=p, b=p):
        return L.esr_bvh_keys(v, nv, t, nf, sb, k, b, null)

    for kw in (dict(nv=-1), dict(nf=-1), dict(v=null), dict(t=null), dict(sb=null), dict(k=null), dict(b=null), dict(v=odd),
               dict(t=odd), dict(sb=odd), dict(k=odd), dict(b=odd2)):
        assert keys(**kw) == -1, kw
    assert keys(nf=big) == -2 and keys(nv=big) == -2 and keys(nf=0, v=null, t=null, sb=null, k=null, b=null) == 0

    def tree(k=p, o=p, nf=4, n=p, lp=p):
        return L.esr_bvh_tree(k, o, nf, n, lp, null)

    for kw in (dict(nf=-1), dict(k=null), dict(o=null), dict(n=null), dict(lp=null), dict(k=odd), dict(o=odd), dict(n=odd8),
               dict(lp=odd2)):
        assert tree(**kw) == -1, kw
    assert tree(nf=big) == -2 and tree(nf=0, k=null, o=null, n=null, lp=null) == 0 and tree(nf=1, k=null, o=null, n=null, lp=null) == 0

    def fit(n=p, lp=p, o=p, b=p, nf=4, c=p, rb=p):
        return L.esr_bvh_fit(n, lp, o, b, nf, c, rb, null)

    for kw in (dict(nf=-1), dict(n=null), dict(lp=null), dict(o=null), dict(b=null), dict(c=null), dict(rb=null), dict(n=odd8),
               dict(lp=odd2), dict(o=odd), dict(b=odd2), dict(c=odd2), dict(rb=odd2)):
        assert fit(**kw) == -1, kw
    assert fit(nf=big) == -2 and fit(nf=0, n=null, lp=null, o=null, b=null, c=null, rb=null) == 0

    def cast(n=p, nf=4, v=p, nv=5, t=p, o=p, d=p, nr=7, lo=null, hi=null, lo_all=0.0, hi_all=math.inf, sk=null, any_hit=0,
             face=p, tt=p, bary=p, hit=null, st=null):
        return L.esr_bvh_cast(n, nf, v, nv, t, o, d, nr, lo, hi, lo_all, hi_all, sk, any_hit, face, tt, bary, hit, st, null)

    for kw in (dict(nf=-1), dict(nv=-1), dict(nr=-1), dict(any_hit=2), dict(any_hit=-1), dict(n=null), dict(v=null), dict(t=null),
               dict(o=null), dict(d=null), dict(face=null), dict(tt=null), dict(bary=null), dict(any_hit=1, hit=null),
               dict(n=odd8), dict(v=odd), dict(t=odd), dict(o=odd), dict(d=odd), dict(lo=odd), dict(hi=odd), dict(sk=odd2),
               dict(face=odd2), dict(tt=odd), dict(bary=odd), dict(st=odd2)):
        assert cast(**kw) == -1, kw
    for kw in (dict(nf=big), dict(nv=big), dict(nr=big)):
        assert cast(**kw) == -2, kw
    assert cast(nr=0, n=null, v=null, t=null, o=null, d=null, face=null, tt=null, bary=null) == 0
