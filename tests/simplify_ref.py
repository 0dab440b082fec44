"""Restatement of mesh.simplify (section S of include/esr_hip.h, the header of csrc/simplify.hip), CPU only.

``grid`` / ``faces``   the clustering and the face rules, literally (numpy integers, a Python dictionary)
``exact``              the per-cluster sums, the solve and the clip in exact rational arithmetic on the float64 inputs
                       r = fl(v - g_k): integers over the cluster's common power-of-two denominator while summing,
                       ``fractions.Fraction`` from there.  Quadrics, c, S, xbar, y and the new vertex are exact.  Only
                       |n| is not rational: w = |n| / 2 is one ``np.longdouble`` square root of the exact n . n (epsilon
                       2^-63, asserted in test_simplify_host.py), and W and P are exact sums of those w.
                       Beside every sum its absref: the same computation on magnitudes (lts_ref64.Q's convention), so
                       that a value is checked as |got - exact| <= K * 2^-53 * absref.
``fast``               the same in vectorised float64 numpy, for the larger cases and the mutants
``emulate``            the kernel's own order of binary64 operations (one lane's loop; 256 strided partial sums and the
                       LDS fold for a cluster of more than ``big`` pairs or members), in Python floats
``check``              every bound of tests/test_gpu_simplify.py, applied to a result (the GPU's or the emulation's)

Bounds (``check``), nothing exempted.  absref of a sum = (the sum of its terms' magnitudes) * (1 + depth), depth being the
longest chain of additions a term passes through in the kernel's order (``depth``: n - 1 for one lane's loop over n
elements, ceil(n / 256) - 1 + 8 for the strided partial sums and the fold): each addition adds at most 2^-53 of a
partial sum, which the magnitudes bound; K covers the roundings that form one term.
  sums      |got - exact| <= K_FAMILY["sums"] * 2^-53 * absref          for A, b, c, S, W
  xbar      |got - exact| <= K_FAMILY["sums"] * 2^-53 * h * (1 + depth of the member sum)       (|r| <= h / 2 for a member)
  position  |got - exact| <= K_FAMILY["pos"] * 2^-53 * (1 + 1 / lam) * h
  attribute |got - P / W| <= 2^-24 |P / W| + 2^-149 + 2 K_FAMILY["sums"] * 2^-53 * (absP / W + |P / W| absW / W): one
            float32 rounding plus the float64 error of the quotient (absP, absW as above); the fallback (W == 0) is exact
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
MAX_CELLS = 2 ** 21 - 1
THREADS = 256
BIG = 64
# The worst ratios |gpu - exact| / (2^-53 scale) measured on the MI355X over every case of tests/test_gpu_simplify.py (printed
# under -s), rounded up to the next power of two.  The emulation of the kernel's order reaches the same ratios (on the CPU
# cases of test_simplify_host.py they seeded the constants before the GPU run) -- the GPU's sums, positions and attributes
# equal it bit for bit.
K_FAMILY = {
    "sums": 4,          # measured worst 2.390 (A, b, c, S, W: a cluster of one or two faces, where absref has no depth to spend;
                        # 0.362 on the marching-cubes sphere, 0.095 on the cluster of 19 602 faces); xbar 0.222
    "pos": 0.25,        # measured worst 0.229 (marching-cubes sphere at 2.5 voxels; cube 0.002, edge cases 0.035)
}
MUTANTS = ("per_corner", "unit_normal", "trace_regulariser", "projection_clamp", "centre_pull", "unweighted_attr")
FACE_MUTANTS = ("keep_degenerate", "keep_duplicates", "keep_later", "normalise_winding", "keep_unreferenced")


def grid(v, h):
    """-> (origin [3], cluster keys [K] ascending, the cluster of every vertex [V], cell centres g [K,3])"""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    h = float(h)
    if not (v.size == 0 or np.isfinite(v).all()):
        raise ValueError("a vertex is not finite")
    if not 0.0 < h < math.inf:
        raise ValueError("cell")
    if v.shape[0] == 0:
        return np.zeros(3), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3))
    o = v.min(0)
    c = np.floor((v - o) / h)
    if c.max() + 1 > MAX_CELLS:
        raise ValueError("too many cells on an axis")
    c = c.astype(np.int64)
    ukeys, vc = np.unique(c[:, 0] << 42 | c[:, 1] << 21 | c[:, 2], return_inverse=True)
    cells = np.stack([ukeys >> 42, (ukeys >> 21) & 0x1fffff, ukeys & 0x1fffff], 1).astype(np.float64)
    return o, ukeys, vc.reshape(-1).astype(np.int64), o + (cells + 0.5) * h


def incident(vc, t, mutant=None):
    """per cluster the incident faces by ascending id, each once (``per_corner``: once per corner in the cluster)"""
    inc = [[] for _ in range(int(vc.max()) + 1 if vc.size else 0)]
    for f, tri in enumerate(np.asarray(t, np.int64).reshape(-1, 3)):
        ks = [int(vc[i]) for i in tri]
        for k in (ks if mutant == "per_corner" else dict.fromkeys(ks)):
            inc[k].append(f)
    return inc


def faces(vc, t, n_clusters, mutant=None):
    """-> (triangles' [F',3], face_origin [F'], new_id [K] (-1: dropped)) by the face rules"""
    t = np.asarray(t, np.int64).reshape(-1, 3)
    seen, kept = {}, []
    for f, tri in enumerate(t):
        ks = tuple(int(vc[i]) for i in tri)
        if len(set(ks)) < 3 and mutant != "keep_degenerate":
            continue
        key = tuple(sorted(ks))
        if key in seen and mutant != "keep_duplicates":
            if mutant == "keep_later":
                kept[seen[key]] = f
            continue
        seen[key] = len(kept)
        kept.append(f)
    kept = sorted(kept)
    origin = np.asarray(kept, np.int64)
    ct = vc[t[origin]].reshape(-1, 3)
    if mutant == "normalise_winding":
        ct = np.sort(ct, 1)
    used = np.zeros(n_clusters, bool)
    used[ct.reshape(-1)] = True
    if mutant == "keep_unreferenced":
        used[:] = True
    new_id = np.where(used, np.cumsum(used) - 1, -1).astype(np.int64)
    return new_id[ct].reshape(-1, 3), origin, new_id


def _frac_ld(x):
    """np.longdouble -> Fraction, exactly"""
    hi = float(x)
    return Fraction(hi) + Fraction(float(x - np.longdouble(hi)))


def _ld_frac(q):
    """Fraction -> np.longdouble, rounded at its precision"""
    hi = float(q)
    return np.longdouble(hi) + np.longdouble(float(q - Fraction(hi)))


def solve_clip(A, b, S, xbar, h, lam, mutant=None):
    """y (three Fractions) from exact A (six), b, S, xbar: the definition's position rule"""
    if S == 0:
        return list(xbar)
    reg = Fraction(lam) * (A[0] + A[3] + A[5] if mutant == "trace_regulariser" else S)
    if reg == 0:
        return list(xbar)
    m = [[A[0] + reg, A[1], A[2]], [A[1], A[3] + reg, A[4]], [A[2], A[4], A[5] + reg]]
    pull = [Fraction(0)] * 3 if mutant == "centre_pull" else xbar
    rhs = [reg * pull[i] - b[i] for i in range(3)]

    def det(c0, c1, c2):
        return (c0[0] * (c1[1] * c2[2] - c1[2] * c2[1]) - c1[0] * (c0[1] * c2[2] - c0[2] * c2[1])
                + c2[0] * (c0[1] * c1[2] - c0[2] * c1[1]))
    cols = [[m[r][c] for r in range(3)] for c in range(3)]
    dd = det(*cols)
    ys = [det(*[rhs if c == i else cols[c] for c in range(3)]) / dd for i in range(3)]
    hh = Fraction(h) / 2
    if mutant == "projection_clamp":
        return [min(max(y, -hh), hh) for y in ys]
    tt = Fraction(1)
    for i in range(3):
        dl = ys[i] - xbar[i]
        if dl > 0:
            tt = min(tt, (hh - xbar[i]) / dl)
        elif dl < 0:
            tt = min(tt, (-hh - xbar[i]) / dl)
    tt = max(tt, Fraction(0))
    return [xbar[i] + tt * (ys[i] - xbar[i]) for i in range(3)]


def quadric_error(A, b, c, y):
    """y^T A y + 2 b . y + c, exactly"""
    m = [[A[0], A[1], A[2]], [A[1], A[3], A[4]], [A[2], A[4], A[5]]]
    return sum(y[i] * m[i][j] * y[j] for i in range(3) for j in range(3)) + 2 * sum(b[i] * y[i] for i in range(3)) + c


class Exact:
    """per cluster: n_pairs, n_members; sums [12] Fractions (A00 A01 A02 A11 A12 A22, b0 b1 b2, c, S, W), absref float64 [K,12], P / absP [K,C],
    xbar, y, pos (three Fractions each), attr: the exact quotient P / W as a Fraction, or the fallback float32 value"""


def exact(v, t, h, lam=1e-3, attr=None):
    v = np.asarray(v, np.float64).reshape(-1, 3)
    t = np.asarray(t, np.int64).reshape(-1, 3)
    o, ukeys, vc, g = grid(v, h)
    n_k, n_c = len(ukeys), 0 if attr is None else attr.shape[1]
    inc = incident(vc, t)
    members = [np.nonzero(vc == k)[0] for k in range(n_k)] if n_k < 64 else None
    if members is None:
        order = np.argsort(vc, kind="stable")
        members = np.split(order, np.cumsum(np.bincount(vc, minlength=n_k))[:-1])
    e = Exact()
    e.origin, e.keys, e.vc, e.g, e.h, e.lam = o, ukeys, vc, g, float(h), float(lam)
    e.n_pairs, e.n_members = [len(fs) for fs in inc], [len(m) for m in members]
    e.sums, e.absref, e.P, e.absP, e.xbar, e.y, e.pos, e.attr, e.fallback = [], np.zeros((n_k, 12)), [], np.zeros((n_k, n_c)), [], [], [], [], []
    hh = Fraction(float(h)) / 2
    for k in range(n_k):
        fs = inc[k]
        rf = v[t[fs]] - g[k] if fs else np.zeros((0, 3, 3))            # [n,3,3]: the float64 inputs
        rm = v[members[k]] - g[k]
        ratios = [float(x).as_integer_ratio() for x in np.concatenate([rf.reshape(-1), rm.reshape(-1)])]
        D = max(d for _, d in ratios)
        ints = [n * (D // d) for n, d in ratios]
        A, b, c, S, W, P = [0] * 6, [0] * 3, 0, 0, Fraction(0), [Fraction(0)] * n_c
        ar = e.absref[k]
        for j, f in enumerate(fs):
            p = [ints[9 * j + 3 * q: 9 * j + 3 * q + 3] for q in range(3)]
            e1, e2 = [p[1][i] - p[0][i] for i in range(3)], [p[2][i] - p[0][i] for i in range(3)]
            n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            d = -(n[0] * p[0][0] + n[1] * p[0][1] + n[2] * p[0][2])
            for q, (i0, i1) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                A[q] += n[i0] * n[i1]
            for i in range(3):
                b[i] += n[i] * d
            c += d * d
            S += sum(x * x for x in e1) * sum(x * x for x in e2)
            nn = Fraction(sum(x * x for x in n), D ** 4)
            w = _frac_ld(np.sqrt(_ld_frac(nn)) / 2)
            ink = [int(vc[i]) == k for i in t[f]]
            W += w * sum(ink)
            # magnitudes, in float64
            x = rf[j]
            f1, f2 = x[1] - x[0], x[2] - x[0]
            an = np.array([abs(f1[1] * f2[2]) + abs(f1[2] * f2[1]), abs(f1[2] * f2[0]) + abs(f1[0] * f2[2]),
                           abs(f1[0] * f2[1]) + abs(f1[1] * f2[0])])
            ad = float(an @ np.abs(x[0]))
            ar[:6] += [an[0] * an[0], an[0] * an[1], an[0] * an[2], an[1] * an[1], an[1] * an[2], an[2] * an[2]]
            ar[6:9] += an * ad
            ar[9] += ad * ad
            ar[10] += float(f1 @ f1) * float(f2 @ f2)
            aw = math.sqrt(float(an @ an)) / 2
            ar[11] += aw * sum(ink)
            for ch in range(n_c):
                P[ch] += w * sum(Fraction(float(attr[i, ch])) for i, inside in zip(t[f], ink) if inside)
                e.absP[k, ch] += aw * sum(abs(float(attr[i, ch])) for i, inside in zip(t[f], ink) if inside)
        A = [Fraction(x, D ** 4) for x in A]
        b = [Fraction(x, D ** 5) for x in b]
        c, S = Fraction(c, D ** 6), Fraction(S, D ** 4)
        nm = len(members[k])
        base = 9 * len(fs)
        xbar = [Fraction(sum(ints[base + 3 * m + i] for m in range(nm)), D * nm) for i in range(3)]
        xbar = [min(max(x, -hh), hh) for x in xbar]
        y = solve_clip(A, b, S, xbar, float(h), float(lam))
        e.sums.append(A + b + [c, S, W])
        e.P.append(P)
        e.xbar.append(xbar)
        e.y.append(y)
        e.pos.append([Fraction(float(g[k, i])) + y[i] for i in range(3)])
        if n_c:
            fb = W == 0
            e.fallback.append(fb)
            e.attr.append([Fraction(float(attr[members[k][0], ch])) if fb else P[ch] / W for ch in range(n_c)])
    return e


def _pairs(vc, t, mutant=None):
    """(cluster, face) incidence pairs, deduplicated per face"""
    t = np.asarray(t, np.int64).reshape(-1, 3)
    ks = vc[t]
    f = np.arange(len(t))
    keep1 = ks[:, 1] != ks[:, 0]
    keep2 = (ks[:, 2] != ks[:, 0]) & (ks[:, 2] != ks[:, 1])
    if mutant == "per_corner":
        keep1 = keep2 = np.ones(len(t), bool)
    return np.concatenate([ks[:, 0], ks[keep1, 1], ks[keep2, 2]]), np.concatenate([f, f[keep1], f[keep2]])


def fast(v, t, h, lam=1e-3, attr=None, mutant=None):
    """float64 numpy form -> dict(sums [K,12], xbar [K,3], pos [K,3], attr float32 [K,C] or None, keys, vc, g)"""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    t = np.asarray(t, np.int64).reshape(-1, 3)
    o, ukeys, vc, g = grid(v, h)
    n_k = len(ukeys)
    pk, pf = _pairs(vc, t, mutant)
    r = v[t[pf]] - g[pk][:, None, :]
    e1, e2 = r[:, 1] - r[:, 0], r[:, 2] - r[:, 0]
    n = np.cross(e1, e2)
    nrm = np.sqrt((n * n).sum(1))
    if mutant == "unit_normal":
        n = n / np.where(nrm > 0, nrm, 1.0)[:, None]
    d = -(n * r[:, 0]).sum(1)
    terms = np.stack([n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1], n[:, 1] * n[:, 2], n[:, 2] * n[:, 2],
                      n[:, 0] * d, n[:, 1] * d, n[:, 2] * d, d * d, (e1 * e1).sum(1) * (e2 * e2).sum(1)], 1)
    ink = vc[t[pf]] == pk[:, None]
    w = np.ones_like(nrm) if mutant == "unweighted_attr" else nrm / 2
    sums = np.zeros((n_k, 12))
    for q in range(11):
        sums[:, q] = np.bincount(pk, terms[:, q], n_k)
    sums[:, 11] = np.bincount(pk, w * ink.sum(1), n_k)
    cnt = np.bincount(vc, minlength=n_k)
    rm = v - g[vc]
    xbar = np.stack([np.bincount(vc, rm[:, i], n_k) for i in range(3)], 1) / cnt[:, None]
    hh = h / 2
    xbar = np.clip(xbar, -hh, hh)
    A = sums[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(n_k, 3, 3)
    S = sums[:, 10]
    reg = lam * (sums[:, 0] + sums[:, 3] + sums[:, 5] if mutant == "trace_regulariser" else S)
    ok = (S > 0) & (reg > 0)
    pull = np.zeros_like(xbar) if mutant == "centre_pull" else xbar
    m = np.where(ok[:, None, None], A + reg[:, None, None] * np.eye(3), np.eye(3))
    ys = np.linalg.solve(m, (reg[:, None] * pull - sums[:, 6:9])[:, :, None])[:, :, 0]
    dl = ys - xbar
    with np.errstate(all="ignore"):
        ta = np.where(dl > 0, (hh - xbar) / dl, np.where(dl < 0, (-hh - xbar) / dl, 1.0))
    tt = np.clip(np.minimum(ta.min(1), 1.0), 0.0, None)
    y = np.clip(ys, -hh, hh) if mutant == "projection_clamp" else xbar + tt[:, None] * dl
    y = np.where(ok[:, None], y, xbar)
    out = dict(sums=sums, xbar=xbar, pos=g + y, attr=None, keys=ukeys, vc=vc, g=g)
    if attr is not None:
        a = np.asarray(attr, np.float32)
        P = np.stack([np.bincount(pk, w * (a[t[pf], ch].astype(np.float64) * ink).sum(1), n_k) for ch in range(a.shape[1])], 1)
        first = np.full(n_k, len(v), np.int64)
        np.minimum.at(first, vc, np.arange(len(v)))
        W = sums[:, 11]
        with np.errstate(all="ignore"):
            out["attr"] = np.where((W > 0)[:, None], P / W[:, None], a[first].astype(np.float64)).astype(np.float32)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel's order, in Python floats (binary64, no contraction)


def _face_terms(p, ink, att):
    """the additions of one incident face: [A00 A01 A02 A11 A12 A22 b0 b1 b2 c S W] and P's, as add_face forms them"""
    e1 = [p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]]
    e2 = [p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]]
    n0 = e1[1] * e2[2] - e1[2] * e2[1]
    n1 = e1[2] * e2[0] - e1[0] * e2[2]
    n2 = e1[0] * e2[1] - e1[1] * e2[0]
    d = -((n0 * p[0][0] + n1 * p[0][1]) + n2 * p[0][2])
    l1 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]
    l2 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2]
    w = math.sqrt((n0 * n0 + n1 * n1) + n2 * n2) * 0.5
    terms = [n0 * n0, n0 * n1, n0 * n2, n1 * n1, n1 * n2, n2 * n2, n0 * d, n1 * d, n2 * d, d * d, l1 * l2, w * float(sum(ink))]
    for row in att:                                                  # one row per channel: the three corners' values
        s = 0.0
        for inside, a in zip(ink, row):
            if inside:
                s += a
        terms.append(w * s)
    return terms


def _fold(partials):
    """block_sum: x[t] += x[t + off] for off = 128 .. 1"""
    x = list(partials)
    off = THREADS // 2
    while off:
        for i in range(off):
            x[i] = x[i] + x[i + off]
        off //= 2
    return x[0]


def _ordered_sum(rows, width, big):
    """column sums of ``rows`` in the kernel's order: serial, or strided partial sums and the fold"""
    if not big:
        acc = [0.0] * width
        for row in rows:
            for q in range(width):
                acc[q] += row[q]
        return acc
    part = [[0.0] * width for _ in range(THREADS)]
    for i, row in enumerate(rows):
        acc = part[i % THREADS]
        for q in range(width):
            acc[q] += row[q]
    return [_fold([p[q] for p in part]) for q in range(width)]


def _finish(A, b, S, M, n_m, h, lam):
    """finish(): -> (xbar, y)"""
    hh = 0.5 * h
    xb = [min(max(M[i] / float(n_m), -hh), hh) for i in range(3)]
    y = list(xb)
    if S > 0.0:
        r = lam * S
        a00, a01, a02, a11, a12, a22 = A[0] + r, A[1], A[2], A[3] + r, A[4], A[5] + r
        r0, r1, r2 = r * xb[0] - b[0], r * xb[1] - b[1], r * xb[2] - b[2]
        l10, l20 = a01 / a00, a02 / a00
        d1 = a11 - l10 * a01
        u12 = a12 - l20 * a01
        l21 = u12 / d1
        d2 = (a22 - l20 * a02) - l21 * u12
        z0 = r0
        z1 = r1 - l10 * z0
        z2 = (r2 - l20 * z0) - l21 * z1
        s2 = z2 / d2
        s1 = z1 / d1 - l21 * s2
        s0 = (z0 / a00 - l10 * s1) - l20 * s2
        dl = [s0 - xb[0], s1 - xb[1], s2 - xb[2]]
        tt = 1.0
        for i in range(3):
            if dl[i] > 0.0:
                tt = min(tt, (hh - xb[i]) / dl[i])
            elif dl[i] < 0.0:
                tt = min(tt, (-hh - xb[i]) / dl[i])
        if not tt >= 0.0:
            tt = 0.0
        for i in range(3):
            val = xb[i] + tt * dl[i]
            y[i] = min(max(val, -hh), hh) if abs(val) < math.inf else xb[i]
    return xb, y


def emulate(v, t, h, lam=1e-3, attr=None, big=BIG):
    """-> dict(sums [K,12], xbar [K,3], pos [K,3], attr float32 [K,C] or None) in the kernel's order of operations"""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    t = np.asarray(t, np.int64).reshape(-1, 3)
    o, ukeys, vc, g = grid(v, h)
    n_k, n_c = len(ukeys), 0 if attr is None else attr.shape[1]
    inc = incident(vc, t)
    order = np.argsort(vc, kind="stable")
    members = np.split(order, np.cumsum(np.bincount(vc, minlength=n_k))[:-1]) if n_k else []
    sums, xbar, pos = np.zeros((n_k, 12)), np.zeros((n_k, 3)), np.zeros((n_k, 3))
    out_attr = np.zeros((n_k, n_c), np.float32) if n_c else None
    for k in range(n_k):
        fs, ms = inc[k], members[k]
        is_big = len(fs) > big or len(ms) > big
        rows = []
        for f in fs:
            p = (v[t[f]] - g[k]).tolist()
            ink = [int(vc[i]) == k for i in t[f]]
            att = [[float(attr[i, ch]) for i in t[f]] for ch in range(n_c)]
            rows.append(_face_terms(p, ink, att))
        q = _ordered_sum(rows, 12 + n_c, is_big)
        M = _ordered_sum((v[ms] - g[k]).tolist(), 3, is_big)
        xb, y = _finish(q[:6], q[6:9], q[10], M, len(ms), float(h), float(lam))
        sums[k], xbar[k] = q[:12], xb
        pos[k] = [float(g[k, i]) + y[i] for i in range(3)]
        for ch in range(n_c):
            out_attr[k, ch] = np.float32(q[12 + ch] / q[11]) if q[11] > 0.0 else attr[ms[0], ch]
    return dict(sums=sums, xbar=xbar, pos=pos, attr=out_attr, keys=ukeys, vc=vc, g=g)


# ---------------------------------------------------------------------------------------------------------------------------
# the bounds


def depth(n, big):
    """the longest chain of additions in the kernel's sum of n elements; ``big``: summed by the workgroup"""
    return (-(-n // THREADS) - 1 + 8 if big else n - 1) if n > 0 else 0


def check(ex, got, what="", big=BIG):
    """Every per-value bound on a result ``got`` (dict: sums [K,12], xbar [K,3], pos [K,3], attr [K,C] or None, all clusters),
    made with the threshold ``big`` (None: no fixed order, as ``fast``: one lane's depth), against ``ex`` (an ``Exact``).
    -> dict of the worst ratios err / bound-without-K per family, and the failures (a list of strings; empty when
    everything holds)."""
    h, lam = ex.h, ex.lam
    worst = dict(sums=0.0, xbar=0.0, pos=0.0, attr=0.0)
    fails = []
    K, KP = K_FAMILY["sums"], K_FAMILY["pos"]
    for k in range(len(ex.sums)):
        is_big = big is not None and (ex.n_pairs[k] > big or ex.n_members[k] > big)
        dp, dm = 1 + depth(ex.n_pairs[k], is_big), 1 + depth(ex.n_members[k], is_big)
        for q in range(12):
            err = abs(Fraction(float(got["sums"][k, q])) - ex.sums[k][q])
            ref = float(ex.absref[k, q]) * dp
            if err == 0:
                continue
            ratio = math.inf if ref == 0.0 else float(err / Fraction(ref)) / U
            worst["sums"] = max(worst["sums"], ratio)
            if not ratio <= K:
                fails.append(f"{what} cluster {k} sum {q}: {ratio:.3g} x 2^-53 absref (K {K})")
        for i in range(3):
            ratio = float(abs(Fraction(float(got["xbar"][k, i])) - ex.xbar[k][i])) / (U * h * dm)
            worst["xbar"] = max(worst["xbar"], ratio)
            if not ratio <= K:
                fails.append(f"{what} cluster {k} xbar {i}: {ratio:.3g} x 2^-53 h (1 + depth) (K {K})")
            ratio = float(abs(Fraction(float(got["pos"][k, i])) - ex.pos[k][i])) / (U * (1.0 + 1.0 / lam) * h)
            worst["pos"] = max(worst["pos"], ratio)
            if not ratio <= KP:
                fails.append(f"{what} cluster {k} position {i}: {ratio:.3g} x 2^-53 (1 + 1 / lam) h (K_POS {KP})")
        if got.get("attr") is not None:
            W = ex.sums[k][11]
            for ch, q in enumerate(ex.attr[k]):
                err = float(abs(Fraction(float(got["attr"][k, ch])) - q))
                if ex.fallback[k]:
                    bound = 0.0
                else:
                    w = float(W)
                    bound = 2.0 ** -24 * abs(float(q)) + 2.0 ** -149 + \
                        2 * K * U * dp * (ex.absP[k, ch] / w + abs(float(q)) * ex.absref[k, 11] / w)
                ratio = 0.0 if err == 0.0 else (math.inf if bound == 0.0 else err / bound)
                worst["attr"] = max(worst["attr"], ratio)
                if not ratio <= 1.0:
                    fails.append(f"{what} cluster {k} attribute {ch}: {ratio:.3g} of its bound")
    return worst, fails


# ---------------------------------------------------------------------------------------------------------------------------
# cases shared by the CPU and the GPU tests


def uv_sphere(n_lat=12, n_lon=16, radius=1.0):
    """a closed triangle sphere: 2 + (n_lat - 1) n_lon vertices, 2 n_lon (n_lat - 1) faces, outward winding"""
    v = [[0.0, 0.0, radius]]
    for i in range(1, n_lat):
        th = math.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * math.pi * j / n_lon
            v.append([radius * math.sin(th) * math.cos(ph), radius * math.sin(th) * math.sin(ph), radius * math.cos(th)])
    v.append([0.0, 0.0, -radius])
    t = []
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon                              # noqa: E731
    for j in range(n_lon):
        t.append([0, ring(1, j), ring(1, j + 1)])
        t.append([len(v) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)])
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            t.append([ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)])
            t.append([ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)])
    return np.asarray(v, np.float64), np.asarray(t, np.int64)


def cube(n=6, side=1.0):
    """a closed cube with sharp edges, n x n quads per side, vertices shared along the edges; outward winding"""
    ids, v, t = {}, [], []

    def vid(p):
        if p not in ids:
            ids[p] = len(v)
            v.append([side * (c / n - 0.5) for c in p])
        return ids[p]
    for axis in range(3):
        for sgn in (0, n):
            for i in range(n):
                for j in range(n):
                    def pt(a, b):
                        p = [0, 0, 0]
                        p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = sgn, a, b
                        return vid(tuple(p))
                    q = [pt(i, j), pt(i + 1, j), pt(i + 1, j + 1), pt(i, j + 1)]
                    if sgn == 0:
                        q.reverse()
                    t += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return np.asarray(v, np.float64), np.asarray(t, np.int64)


def attributes(v, n_c, seed=0):
    """float32 [V, n_c]: smooth functions of the position and one noisy, one signed and one constant channel"""
    rng = np.random.default_rng(seed)
    a = np.stack([np.sin(3.0 * v[:, i % 3] + i) for i in range(n_c)], 1)
    a[:, 0] = rng.standard_normal(len(v))
    if n_c > 2:
        a[:, 1] = np.abs(a[:, 1]) * 1e3
        a[:, 2] = 0.25
    return a.astype(np.float32)


def edge_case(name):
    """-> (vertices, triangles, h): the exact edge cases of the definition"""
    if name == "collinear_and_coincident":
        # face 2 is collinear: the smallest coordinate is 0.125 on every axis and vertices 5, 6, 7 are dyadic, so their
        # r = v - g is exact and n is exactly 0 (s > 0); face 3 has two coincident corners (s == 0)
        v = [[0.125, 0.125, 0.125], [0.9, 0.15, 0.2], [0.2, 0.8, 0.3], [1.3, 0.2, 0.15], [1.7, 0.9, 0.35], [0.25, 0.375, 0.25],
             [0.5, 0.5, 0.5], [0.75, 0.625, 0.75], [0.2, 0.8, 0.3], [1.2, 1.4, 0.2], [0.3, 1.6, 0.15]]
        t = [[0, 1, 2], [1, 3, 4], [5, 6, 7], [2, 8, 4], [2, 4, 9], [2, 9, 10], [1, 4, 2]]
        return np.asarray(v, np.float64), np.asarray(t, np.int64), 1.0
    if name == "all_degenerate_cluster":
        # cluster of vertices 3, 4 (x in [2, 3)) meets only faces with coincident corners: S == 0, W == 0 there
        v = [[0.1, 0.2, 0.1], [0.8, 0.3, 0.2], [0.3, 0.9, 0.4], [2.5, 0.5, 0.5], [2.5, 0.5, 0.5], [2.25, 0.75, 0.25], [1.5, 0.5, 0.5]]
        t = [[0, 1, 2], [3, 4, 5], [3, 4, 3], [5, 5, 4]]
        return np.asarray(v, np.float64), np.asarray(t, np.int64), 1.0
    if name == "two_sheets":
        # faces 0 and 1 fall on the same three clusters with opposite winding (face 0 stays); face 2 repeats face 0's
        # triple rotated; face 3 is another triple
        v = [[0.2, 0.2, 0.2], [1.3, 0.2, 0.3], [0.3, 1.4, 0.2], [0.25, 0.3, 0.6], [1.4, 0.3, 0.7], [0.2, 1.3, 0.6],
             [1.6, 1.6, 0.4], [0.4, 0.1, 0.1]]
        t = [[0, 1, 2], [3, 5, 4], [1, 2, 7], [1, 6, 2]]
        return np.asarray(v, np.float64), np.asarray(t, np.int64), 1.0
    if name == "on_cell_borders":
        # every coordinate is a multiple of h / 2 = 0.25: a vertex sits on the lower border of its cell or in its middle, and
        # the vertices of the far sides (coordinate 1 = 2 h) open a layer of cells of their own
        v, t = cube(4, 1.0)
        return v, t, 0.5
    if name == "one_cell":
        v, t = uv_sphere(6, 8)
        return v, t, 8.0
    if name == "no_faces":
        return np.asarray([[0.0, 0.0, 0.0], [0.3, 0.1, 0.2], [1.5, 0.2, 0.1], [1.6, 1.7, 0.3]]), np.zeros((0, 3), np.int64), 1.0
    raise KeyError(name)


EDGE_CASES = ("collinear_and_coincident", "all_degenerate_cluster", "two_sheets", "on_cell_borders", "one_cell", "no_faces")


def dense_patch(n=100, seed=3):
    """a bumpy n x n height-field patch inside one cell: 2 (n - 1)^2 faces on n^2 vertices (the large-cluster case)"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.linspace(0.05, 0.9, n), np.linspace(0.1, 0.95, n), indexing="ij")
    z = 0.5 + 0.2 * np.sin(5 * x) * np.cos(4 * y) + 0.01 * rng.standard_normal((n, n))
    v = np.stack([x, y, z], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).reshape(-1)
    t = np.concatenate([np.stack([a, a + n, a + n + 1], 1), np.stack([a, a + n + 1, a + 1], 1)])
    return v, t.astype(np.int64)
