"""Restatement of the surface lighting (esr_nerf_amd/csrc/surflight.hip, sources.source_lights / direct_light / lit_view):
section U of include/esr_hip.h taken word by word in numpy, with none of the kernel's machinery; never imported by the product.

  lights       the slot-major light arrays in a direct float64 loop over the sources (the rule of sources.source_lights)
  emulate      the kernel's ORDER of operations: binary64 for the geometry and the balanced pairwise sum (numpy rounds every
               operation on its own), binary32 for the BRDF (lts_ref64._disney in mode "32": every operation a separately
               rounded binary32 one); visibility from raycast_ref.brute with its `ambiguous` flag.  Its mutants stand for the
               mistakes a kernel of this kind can make
  reference    mode 1: the same quantity in extended precision (np.longdouble) with `absref`, the sum over the slots of the
               term's magnitude with every dot product taken over absolute values;  mode 0: the BRDF through lts_ref64's
               value-and-error pairs Q at the binary32-rounded w, absref = sum_k E_k c_k + |sum| (the final rounding) + the
               binary64 chain's share
  check        the checks of tests/test_gpu_surflight.py on one case: the emulation passes them (test_surflight_host.py) and
               every mutant fails one

Bounds.
  mode 1   out is BIT-EQUAL to the emulation: the binary32 rounding of the emulation's binary64 sum.  A binary32 number cannot
           lie within 2^-53 of anything, so it is that binary64 sum which is held against extended precision:
           |sum64 - ref| <= K_IRR 2^-53 absref.  K_IRR is the worst ratio over every case of the CPU and GPU tests (the two
           are the same numbers, the GPU being bit-equal), rounded up to the next integer.
  mode 0   |gpu - ref| <= K_FAMILY["reflect"] 2^-24 absref, K by the rule of lts_ref64.K_FAMILY (the next power of two at or
           above twice the measured worst ratio).  The kernel's disney_eval is compiled as lts.hip compiles it, with
           contraction: a * b + c may round once where the emulation rounds twice, so the GPU is not bit-equal to the
           emulation in this mode and its worst ratio differs from the emulation's in the second digit.
"""
import math

import numpy as np
import torch

import lts_ref64 as lr
import raycast_ref as rr

U53, U24 = 2.0 ** -53, 2.0 ** -24
K_T = rr.K_T             # the walk's own bound on t (raycast_ref), unchanged here
K_IRR = 2                # mode 1: measured worst |sum64 - ref| / (2^-53 absref) 1.18 (the one-face mesh; the second grid trip 1.09) over every case of the CPU and GPU tests
K_FAMILY = {
    "reflect": 1,        # mode 0: measured worst 0.231 on the MI355X (S = 2; the emulation reaches 0.286 there: contraction); room/16 0.199 on both
}
INV2PI = 1.0 / (2.0 * math.pi)
MAX_SLOTS = 64

MUTANTS = ("no_inv2pi", "no_r2_clamp", "clamp_wrong_area", "back_face_emits", "cos_from_face_normal", "area_over_K",
           "serial_sum", "sources_swapped", "skip_ignored", "eps_zero", "w_unnormalised")


# ----------------------------------------------------------------------------------------------------------------------
# scenes: (v, tr, face_source, n_sources)


def refined_room(m):
    """raycast_ref.room() with every quad split m x m (its two faces become 2 m m): the ceiling patch has 4 m m faces"""
    v0, t0, s0, S = rr.room()
    v, t, src = [], [], []
    for q in range(0, len(t0), 2):
        a, b, c, d = (v0[i] for i in (t0[q][0], t0[q][1], t0[q][2], t0[q + 1][2]))
        for i in range(m):
            for j in range(m):
                base = len(v)
                for (fu, fw) in ((i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1)):
                    v.append(a + (b - a) * (fu / m) + (d - a) * (fw / m))
                t.extend([(base, base + 1, base + 2), (base, base + 2, base + 3)])
                src.extend([s0[q]] * 2)
    return np.array(v, np.float64), np.array(t, np.int64), np.array(src, np.int32), S


def square(n=8, side=1.0, occluder=False):
    """one emissive square [-side/2, side/2]^2 in the plane z = 0 facing +z, n x n quads on shared vertices (2 n n faces, all of
    source 0); with `occluder` one more face, not emissive, hanging over a corner of it"""
    g = np.linspace(-0.5, 0.5, n + 1) * side
    v = [(x, y, 0.0) for y in g for x in g]
    t = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            t.extend([(a, a + 1, a + n + 2), (a, a + n + 2, a + n + 1)])
    src = [0] * len(t)
    if occluder:
        b = len(v)
        v.extend([(0.05 * side, 0.07 * side, 0.3 * side), (0.62 * side, 0.11 * side, 0.3 * side), (0.31 * side, 0.66 * side, 0.35 * side)])
        t.append((b, b + 1, b + 2))
        src.append(-1)
    return np.array(v, np.float64), np.array(t, np.int64), np.array(src, np.int32), 1


def vertex_emission(v, tr, fs, seed=0):
    """float32 [V, 3]: 0.5 .. 4 at the vertices of source faces, 0 elsewhere"""
    rng = np.random.default_rng(seed)
    em = np.zeros((len(v), 3), np.float32)
    hot = np.unique(np.asarray(tr)[np.asarray(fs) >= 0])
    em[hot] = rng.uniform(0.5, 4.0, (len(hot), 3)).astype(np.float32)
    return em


def closed_form_square(side, h, E=1.0):
    """the irradiance on a plane parallel to a square Lambertian emitter of radiance E, on its axis at height h: pi E times
    the view factor of the four corner rectangles X = Y = (side / 2) / h"""
    X = Y = (side / 2.0) / h
    F = (1.0 / (2.0 * math.pi)) * (X / math.sqrt(1 + X * X) * math.atan(Y / math.sqrt(1 + X * X)) +
                                  Y / math.sqrt(1 + Y * Y) * math.atan(X / math.sqrt(1 + Y * Y)))
    return math.pi * E * 4.0 * F


# ----------------------------------------------------------------------------------------------------------------------
# the lights


def next_pow2(n):
    k = 1
    while k < n:
        k *= 2
    return k


def face_normals(v, tr, ids):
    """(n [k, 3] not normalised, |n| [k]) of the faces `ids`, every operation on its own"""
    v, tr = np.asarray(v, np.float64), np.asarray(tr, np.int64)
    a, b, c = (v[tr[ids, k]] for k in range(3))
    e1, e2 = b - a, c - a
    n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return np.stack([n0, n1, n2], 1), np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)


def lights(v, tr, fs, S, samples, emission, area=None, mutant=None):
    """dict(point [S, Kp, 3], normal, weight [S, Kp], radiance f32 [S, Kp, 3], face i32 [S, Kp], n [S], area [S]): one source
    and one sample at a time.  `area` [S]: the sources' areas where the caller has them (SourceReport.area); else the sum
    of the faces' areas in id order"""
    faces, points, _ = rr.source_samples(v, tr, fs, S, samples)
    kp = next_pow2(samples)
    L = dict(point=np.zeros((S, kp, 3)), normal=np.zeros((S, kp, 3)), weight=np.zeros((S, kp)),
             radiance=np.zeros((S, kp, 3), np.float32), face=np.full((S, kp), -1, np.int32), n=np.zeros(S, np.int64),
             area=np.zeros(S))
    third = np.float32(1.0 / 3.0)
    for s in range(S):
        ids = np.flatnonzero(np.asarray(fs) == s)
        _, ln = face_normals(v, tr, ids)
        total = float(area[s]) if area is not None else float(np.cumsum(ln * 0.5)[-1])
        n = len(faces[s])
        L["n"][s], L["area"][s] = n, total
        for k in range(n):
            f = int(faces[s][k])
            nv, ln = face_normals(v, tr, np.array([f]))
            L["point"][s, k] = points[s][k]
            L["normal"][s, k] = nv[0] / ln[0]
            L["weight"][s, k] = total / (samples if mutant == "area_over_K" else n)
            e = [np.asarray(emission, np.float32)[tr[f, j]] for j in range(3)]
            L["radiance"][s, k] = ((e[0] + e[1]) + e[2]) * third
            L["face"][s, k] = f
    return L


# ----------------------------------------------------------------------------------------------------------------------
# the kernel's order of operations


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _disney(mat, idx, wi32, mode):
    """R [N, 3] of the live entries idx = (p, s, k): lts_ref64._disney in the number system `mode` ("32": a torch binary32
    tensor, "q": value-and-error pairs)"""
    p = idx[0]
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    a, ro, m = lr.lift(T(mat["base"][p])[:, None, :], mode), lr.lift(T(mat["rough"][p])[:, None], mode), lr.lift(T(mat["metal"][p])[:, None], mode)
    n, wo = lr.lift(T(mat["normal"][p])[:, None, :], mode), lr.lift(T(mat["wo"][p])[:, None, :], mode)
    wi = lr.lift(T(wi32)[:, None, :], mode)
    R = lr._disney(a, ro, m, n, wi, wo, mode)
    return R.reshape(len(p), 3) if isinstance(R, lr.Q) else R.reshape(len(p), 3)


def emulate(case, mutant=None):
    """-> dict(out f32 [P, S, 3], sum64 [P, S, 3], seen u8 [P, S, Kp], ambiguous bool [P, S, Kp], parts ...) of a case
    dict(v, tr, L, pts f64 [P, 3], nrm f32 [P, 3], mode, eps, mat = dict(base, rough, metal, wo: f32) in mode 0)"""
    v, tr, L, mode = case["v"], case["tr"], case["L"], case["mode"]
    eps = 0.0 if mutant == "eps_zero" else case["eps"]
    x = np.asarray(case["pts"], np.float64)[:, None, None, :]
    nrm = np.asarray(case["nrm"], np.float32)
    P, (S, kp) = x.shape[0], L["weight"].shape
    with np.errstate(all="ignore"):
        d = L["point"][None] - x
        r2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        r = np.sqrt(r2)
        w = d / r[..., None]
        g = np.broadcast_to(L["normal"][None], d.shape)
        cos_l = -_dot(g, w)
        n_used = case["face_nrm"] if mutant == "cos_from_face_normal" else nrm
        cos_x = _dot(n_used.astype(np.float64)[:, None, None, :], w)
        A = np.broadcast_to(L["weight"][None], r2.shape)
        if mutant == "back_face_emits":
            cos_l = np.abs(cos_l)
        live = (A != 0.0) & (r2 > 0.0) & (cos_l > 0.0) & (cos_x > 0.0)
        clamp = np.broadcast_to(L["area"][None, :, None], r2.shape) if mutant == "clamp_wrong_area" else A
        G = (cos_l * A) / (r2 if mutant == "no_r2_clamp" else np.fmax(r2, clamp))
    idx = np.nonzero(live)
    seen = np.zeros((P, S, kp), np.uint8)
    amb = np.zeros((P, S, kp), bool)
    if len(idx[0]):
        o = np.broadcast_to(x, d.shape)[idx]
        skip = np.full(len(idx[0]), -1, np.int64) if mutant == "skip_ignored" else L["face"][idx[1], idx[2]].astype(np.int64)
        b = rr.brute(v, tr, o, d[idx], eps, 1.0 - eps, skip)
        seen[idx] = np.where(b["hit"], 2, 1)
        amb[idx] = b["ambiguous"]
    term = np.zeros((P, S, kp, 3))
    vis = np.nonzero(seen == 1)
    E = L["radiance"][vis[1], vis[2]].astype(np.float64)
    parts = dict(vis=vis, G=G[vis], w=w[vis], cos_x=cos_x[vis], E=E, live=live,
                 Gabs=(_dot(np.abs(g), np.abs(w)) * A / np.fmax(r2, A))[vis] if len(vis[0]) else np.zeros(0),
                 cos_x_abs=_dot(np.abs(nrm.astype(np.float64))[:, None, None, :], np.abs(w))[vis] if len(vis[0]) else np.zeros(0))
    if len(vis[0]):
        if mode == 0:
            wi = (d[vis] if mutant == "w_unnormalised" else w[vis]).astype(np.float32)
            R = _disney(dict(case["mat"], normal=nrm), vis, wi, "32").numpy().astype(np.float64)
            f = 1.0 if mutant == "no_inv2pi" else INV2PI
            term[vis] = ((R * f) * G[vis][:, None]) * E
        else:
            term[vis] = (cos_x[vis] * G[vis])[:, None] * E
    t = term
    if mutant == "serial_sum":
        acc = t[:, :, 0]
        for k in range(1, kp):
            acc = acc + t[:, :, k]
        t = acc[:, :, None]
    while t.shape[2] > 1:
        t = t[:, :, 0::2] + t[:, :, 1::2]
    sum64 = t[:, :, 0]
    if mutant == "sources_swapped":
        sum64, seen = sum64[:, ::-1], seen[:, ::-1]
    with np.errstate(over="ignore"):
        return dict(out=sum64.astype(np.float32), sum64=sum64, seen=seen, ambiguous=amb, parts=parts)


def reference(case, emu):
    """(value f64 [P, S, 3], absref [P, S, 3]) with the emulation's decisions (which slots are silent, which are shadowed)"""
    L, mode, pr = case["L"], case["mode"], emu["parts"]
    vis = pr["vis"]
    P, (S, kp) = len(case["pts"]), L["weight"].shape
    val, absref = np.zeros((P, S, kp, 3)), np.zeros((P, S, kp, 3))
    if len(vis[0]):
        if mode == 1:
            X = np.longdouble
            x, y = np.asarray(case["pts"], np.float64)[vis[0]].astype(X), L["point"][vis[1], vis[2]].astype(X)
            g, n = L["normal"][vis[1], vis[2]].astype(X), np.asarray(case["nrm"], np.float32)[vis[0]].astype(X)
            A = L["weight"][vis[1], vis[2]].astype(X)
            d = y - x
            r2 = (d * d).sum(-1)
            w = d / np.sqrt(r2)[:, None]
            G = -(g * w).sum(-1) * A / np.maximum(r2, A)
            val[vis] = ((n * w).sum(-1) * G)[:, None].astype(np.float64) * pr["E"]
            absref[vis] = (pr["cos_x_abs"] * pr["Gabs"])[:, None] * np.abs(pr["E"])
        else:
            R = _disney(dict(case["mat"], normal=np.asarray(case["nrm"], np.float32)), vis, pr["w"].astype(np.float32), "q")
            c = (INV2PI * pr["G"])[:, None] * pr["E"]
            val[vis] = R.v.numpy() * c
            # E_k c_k, and the binary64 chain (under 64 roundings of 2^-53 on magnitudes: 64 2^-29 in units of 2^-24)
            absref[vis] = R.E.numpy() * np.abs(c) + 64 * 2.0 ** -29 * np.abs(R.v.numpy()) * (INV2PI * pr["Gabs"])[:, None] * np.abs(pr["E"])
    value = val.sum(2)
    absref = absref.sum(2) + (np.abs(val).sum(2) * (kp.bit_length()) if mode == 1 else np.abs(value))
    return value, absref


def check(case, out, seen=None, emu=None, what=""):
    """The GPU's checks of one case -> (worst ratio, ambiguous count); raises AssertionError.  `out` f32 [P, S, 3]"""
    emu = emu or emulate(case)
    out = np.asarray(out)
    assert out.dtype == np.float32 and out.shape == emu["out"].shape, (what, out.dtype, out.shape)
    clear = ~emu["ambiguous"].any(2)                                      # (p, s) whose every segment is unambiguous
    value, absref = reference(case, emu)
    if case["mode"] == 1:
        bad = np.argwhere((out.view(np.uint32) != emu["out"].view(np.uint32)).any(-1) & clear)
        assert len(bad) == 0, (what, "mode 1 is not bit-equal to the binary64 emulation", len(bad), bad[:4].tolist(),
                               [out[p, s].tolist() for p, s in bad[:4]], [emu["out"][p, s].tolist() for p, s in bad[:4]])
        err, unit, K = np.abs(emu["sum64"] - value), U53, K_IRR
    else:
        err, unit, K = np.abs(out.astype(np.float64) - value), U24, K_FAMILY["reflect"]
    ratio = np.where(absref > 0, err / np.maximum(unit * absref, 1e-300), np.where(err > 0, np.inf, 0.0))[clear]
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= K, (what, "the bound does not hold", worst, K)
    if seen is not None:
        seen = np.asarray(seen)
        assert seen.dtype == np.uint8 and seen.shape == emu["seen"].shape, (what, seen.dtype, seen.shape)
        ok = ~emu["ambiguous"]
        assert np.array_equal(seen[ok], emu["seen"][ok]), (what, "seen differs on unambiguous segments", int((seen != emu["seen"])[ok].sum()))
    return worst, int(emu["ambiguous"].sum())


# ----------------------------------------------------------------------------------------------------------------------
# points and cases


def unit32(n):
    n = np.asarray(n, np.float32)
    return (n / np.sqrt((n * n).sum(-1, keepdims=True, dtype=np.float32))).astype(np.float32)


def materials(P, pts, seed, eye=(2.1, 1.4, 1.2)):
    """base, rough, metal and wo (unit, towards `eye`) of P points"""
    rng = np.random.default_rng(seed)
    wo = unit32(np.asarray(eye)[None] - np.nan_to_num(np.asarray(pts, np.float64)))
    return dict(base=rng.uniform(0.1, 0.9, (P, 3)).astype(np.float32), rough=rng.uniform(0.15, 0.95, P).astype(np.float32),
                metal=rng.uniform(0.0, 1.0, P).astype(np.float32), wo=wo)


def points_on_faces(v, tr, n, seed, tilt=0.0):
    """(points on n random faces well inside them, their shading normals f32, the faces' unit normals f32): the normal is
    the face's, turned towards the room's middle, tilted by up to `tilt`"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, len(tr), n)
    b = rng.uniform(0.15, 0.7, (n, 2))
    b = np.where(b.sum(1, keepdims=True) > 0.85, b * 0.5, b)
    a, bb, c = (np.asarray(v)[np.asarray(tr)[ids, k]] for k in range(3))
    pts = a * (1 - b[:, :1] - b[:, 1:]) + bb * b[:, :1] + c * b[:, 1:]
    nv, ln = face_normals(v, tr, ids)
    fn = nv / ln[:, None]
    mid = np.asarray(v).mean(0)
    fn = np.where(((mid[None] - pts) * fn).sum(1, keepdims=True) < 0, -fn, fn)
    sn = fn + tilt * rng.uniform(-1, 1, (n, 3))
    return pts, unit32(sn), unit32(fn)


def make_case(scene, samples, pts, nrm, mode, eps=1e-6, seed=0, face_nrm=None, L=None, mutant=None):
    v, tr, fs, S = scene
    if L is None:
        L = lights(v, tr, fs, S, samples, vertex_emission(v, tr, fs, seed), mutant=mutant)
    case = dict(v=v, tr=tr, fs=fs, L=L, pts=np.asarray(pts, np.float64), nrm=np.asarray(nrm, np.float32), mode=mode, eps=eps,
                face_nrm=np.asarray(nrm if face_nrm is None else face_nrm, np.float32))
    if mode == 0:
        case["mat"] = materials(len(pts), pts, seed + 1)
    return case


def special_points(scene, L):
    """points coplanar with source 0 (the cosine at the source is exactly 0), a point AT a sample (r2 = 0), a point with a NaN
    coordinate, and one behind the source; with a normal that faces the source where there is a side to face"""
    y, g = L["point"][0, 0], L["normal"][0, 0]
    axis = int(np.argmax(np.abs(g)))
    side = np.zeros(3)
    side[(axis + 1) % 3] = 1.0
    pts = [y + 0.37 * side, y - 1.9 * side, y.copy(), np.array([np.nan, 1.0, 1.0]), y + 0.5 * g + 0.1 * side, y - 0.4 * g]
    nrm = [-side, side, g, g, -g, g]
    return np.array(pts), unit32(np.array(nrm))


def room_cases(mode):
    """name -> case: the generic cases of the room and its refinements, and the special points.  The points on faces take
    eps = 1e-3: the face a point lies on is met at t = 0 up to rounding, which raycast_ref.brute calls ambiguous beside
    a t_min of 1e-6 (its resolution KEY_RES is 2^-22)"""
    room = rr.room()
    up = unit32(np.tile([[0.0, 0.0, 1.0]], (len(rr.room_points()), 1)))
    side = unit32(np.tile([[-0.6, 0.1, 0.8]], (len(rr.room_points()), 1)))
    cases = {"room/16": make_case(room, 16, rr.room_points(), up, mode),
             "room/3 tilted": make_case(room, 3, rr.room_points(), side, mode, face_nrm=up)}
    for m, samples in ((2, 16), (4, 64)):
        sc = refined_room(m)
        p, sn, fn = points_on_faces(sc[0], sc[1], 12, 10 + m, tilt=0.0 if m == 2 else 0.4)
        cases[f"room x{m}/{samples} on faces"] = make_case(sc, samples, p, sn, mode, eps=1e-3, seed=m, face_nrm=fn)
    sp, sn = special_points(room, cases["room/16"]["L"])
    cases["room/16 special"] = make_case(room, 16, sp, sn, mode, L=cases["room/16"]["L"])
    return cases


def tie_case():
    """One point, one source of four slots, no face: every slot at distance exactly 2 straight over the point with A = 1, so
    that G = 1/4 and the terms are E / 4 without a rounding: 1, 2^-24, 3/4 2^-53, 3/4 2^-53.  The pairwise sum
    (1 + 2^-24) + 3/2 2^-53 rounds UP in binary64 and then up in binary32 (1 + 2^-23); a serial sum drops both small terms,
    stays on the binary32 tie 1 + 2^-24 and rounds to even, 1: the one output value shows the order of the sum"""
    L = dict(point=np.zeros((1, 4, 3)), normal=np.tile([0.0, 0.0, 1.0], (1, 4, 1)), weight=np.ones((1, 4)),
             radiance=np.tile(np.array([4.0, 2.0 ** -22, 3 * 2.0 ** -53, 3 * 2.0 ** -53], np.float32)[None, :, None], (1, 1, 3)),
             face=np.full((1, 4), -1, np.int32), n=np.full(1, 4, np.int64), area=np.full(1, 4.0))
    scene = (np.zeros((3, 3)), np.zeros((0, 3), np.int64), np.zeros(0, np.int32), 1)
    return make_case(scene, 4, np.array([[0.0, 0.0, 2.0]]), np.array([[0.0, 0.0, -1.0]], np.float32), 1, L=L)


def square_case(h, samples=64, n=8, side=1.0, E=1.0):
    """the irradiance of the n x n-quad square of radiance E at the point on its axis at height h * side"""
    sc = square(n, side)
    em = np.full((len(sc[0]), 3), E, np.float32)
    L = lights(sc[0], sc[1], sc[2], 1, samples, em)
    return make_case(sc, samples, np.array([[0.0, 0.0, h * side]]), np.array([[0.0, 0.0, -1.0]], np.float32), 1, L=L)
