"""Section W of include/esr_hip.h (the texture atlas of csrc/atlas.hip) restated in numpy: the integer layout, the binary64
arithmetic in the kernels' operation order (numpy rounds every elementwise operation once and contracts nothing, so the bits
are the kernels'), and the binary32 blends.  Every function takes ``mutant``: one of MUTANTS changes the one thing its name
says, and tests/test_atlas_host.py shows that the checks of this file (``check_*``: brute force from the definitions, written
independently of the restatement) reject each of them.

The end-to-end property.  Vertex attributes baked without a model and looked up again at a point of a face equal the
barycentric interpolation of the attributes within K 2^-24 absref, absref = the bilinear blend of the four texels'
sum_k |w_k| |attr_k| (w_k: the texel's affine weights, which leave [0, 1] in the gutter).  The worst ratios found, over the cases
of tests/test_gpu_atlas.py (64 random points plus the corners and edge midpoints of every face, 12 channels):
    the emulation of this file   WORST_EMULATION = 32.292 (the marching-cubes sphere; 20.997 on the other cases)
    the MI355X                   WORST_MI355X = 32.292    (its texels and samples are bit-equal to the emulation, so the same
                                                          points give the same ratio)
K = 64 is the smallest power of two at or above the larger of the two.  Why the ratio is not a small constant: the texel pass
forms the first weight in binary32 as (1 - beta) - gamma, so that weight carries an absolute error of about 2^-24 (|beta| +
|gamma|) even where it vanishes itself -- on the edge opposite the first corner.  There the error is 2^-24 |attr_a| while absref
holds only |attr_b| and |attr_c|: the ratio follows |attr_a| / (|attr_b| + |attr_c|), and the normally distributed test
attributes reach 32 somewhere among 2.7 million values.  For attributes of one sign and similar size (uniform in [0.25, 1], as colours and roughness
are) the emulation's worst ratio on the cube, far-faces and level-span cases is 4.36.
"""
import numpy as np

MUTANTS = ("halves_swapped", "diagonal_to_wrong_half", "rot_ignored", "leg_off_by_one", "ascending_levels", "unstable_ties",
           "morton_xy_swapped", "clamped_barycentrics", "odd_tail_mapped", "half_texel_dropped", "weights_wrong_axis")
WORST_EMULATION = 32.292
WORST_MI355X = 32.292
K = 64.0
NL = 16


def low_level(g):
    """the smallest l with 2^l >= 3 g + 2"""
    l = 0
    while (1 << l) < 3 * g + 2:
        l += 1
    return l


def leg(l, g, mutant=None):
    return (1 << l) - (3 * g + 1) - (1 if mutant == "leg_off_by_one" else 0)


def owner(i, j, s, mutant=None):
    """the half that owns the local texel (i, j) of a cell of side s"""
    return int(i + j > s - 1 - (1 if mutant == "diagonal_to_wrong_half" else 0))


def triangle(l, g, half, mutant=None):
    """a, b, c of the half's UV triangle in local texel units (integers)"""
    s, e = 1 << l, leg(l, g, mutant)
    if mutant == "halves_swapped":
        half = 1 - half
    if half == 0:
        return np.array([[g, g], [g + e, g], [g, g + e]], dtype=np.int64)
    return np.array([[s - g, s - g], [s - g - e, s - g], [s - g, s - g - e]], dtype=np.int64)


def footprint(p):
    """the four local texels a bilinear lookup at the point p (texel units, exact rationals or floats) touches"""
    i0, j0 = int(np.floor(p[0] - 0.5)), int(np.floor(p[1] - 0.5))
    return [(i0, j0), (i0 + 1, j0), (i0, j0 + 1), (i0 + 1, j0 + 1)]


# ---------------------------------------------------------------- levels

def levels(v, t, g, lmin, lmax, rho4, mutant=None):
    """-> level int32 [F], rot int32 [F], hist int64 [16]"""
    v, t = np.asarray(v, np.float64).reshape(-1, 3), np.asarray(t, np.int64).reshape(-1, 3)
    F = len(t)
    ok = ((t >= 0) & (t < len(v))).all(axis=1) if F else np.zeros(0, bool)
    tt = np.where(ok[:, None], t, 0) if len(v) else np.zeros_like(t)
    vv = v if len(v) else np.zeros((1, 3))
    with np.errstate(all="ignore"):
        a, b, c = vv[tt[:, 0]], vv[tt[:, 1]], vv[tt[:, 2]]
        e1, e2, e0 = b - a, c - a, c - b
        n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        c2 = (n0 * n0 + n1 * n1) + n2 * n2
        need = c2 * np.float64(rho4)
        level = np.full(F, lmax, np.int32)
        done = np.zeros(F, bool)
        for l in range(lmin, lmax):
            e = np.float64(leg(l, g, mutant) ** 2)
            hit = ~done & (e * e >= need)
            level[hit], done = l, done | hit
        level[~np.isfinite(c2)] = lmin
        d = [(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2] for e in (e0, e2, e1)]
        rot = np.zeros(F, np.int32)
        best = d[0].copy()
        m = d[1] > best
        rot[m], best = 1, np.where(m, d[1], best)
        rot[d[2] > best] = 2
    level[~ok], rot[~ok] = lmin, 0
    return level, rot, np.bincount(level, minlength=NL).astype(np.int64)


def sort_order(level, lmax, mutant=None):
    level = np.asarray(level, np.int64)
    if mutant == "ascending_levels":
        return np.argsort(level, kind="stable")
    if mutant == "unstable_ties":
        return np.lexsort((-np.arange(len(level)), lmax - level))
    return np.argsort(lmax - level, kind="stable")


def groups(counts, lmin, lmax):
    """-> (start, unit, cells) int64 [16] each, and the units used"""
    start, unit, cells = np.zeros(NL, np.int64), np.zeros(NL, np.int64), np.zeros(NL, np.int64)
    s = u = 0
    for l in range(lmax, lmin - 1, -1):
        start[l], unit[l], cells[l] = s, u, (int(counts[l]) + 1) // 2
        s += int(counts[l])
        u += int(cells[l]) << (2 * (l - lmin))
    return start, unit, cells, u


def fits(counts, W, lmin, lmax):
    return groups(counts, lmin, lmax)[3] <= (W >> lmin) ** 2


def morton_decode(u, mutant=None):
    """even bits -> x, odd bits -> y"""
    u = np.asarray(u, np.int64)
    x, y = np.zeros_like(u), np.zeros_like(u)
    for b in range(16):
        x |= ((u >> (2 * b)) & 1) << b
        y |= ((u >> (2 * b + 1)) & 1) << b
    return (y, x) if mutant == "morton_xy_swapped" else (x, y)


def morton_encode(x, y, mutant=None):
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    if mutant == "morton_xy_swapped":
        x, y = y, x
    m = np.zeros_like(x)
    for b in range(16):
        m |= ((x >> b) & 1) << (2 * b) | ((y >> b) & 1) << (2 * b + 1)
    return m


def interleave(x, y):
    """an independent bit interleave (through binary strings), for the test of the two functions above"""
    bx, by = format(int(x), "016b"), format(int(y), "016b")
    return int("".join(q + p for p, q in zip(bx, by)), 2)


def charts(order, level, rot, counts, W, g, lmin, lmax, mutant=None):
    """-> chart int32 [F, 4], uv float32 [F, 3, 2]"""
    order = np.asarray(order, np.int64)
    F = len(order)
    start, unit, _, _ = groups(counts, lmin, lmax)
    chart, uv = np.zeros((F, 4), np.int32), np.zeros((F, 3, 2), np.float32)
    k = np.arange(F, dtype=np.int64)
    lv = np.full(F, lmin, np.int64)
    for l in range(lmax, lmin, -1):
        lv[(k >= start[l]) & (k < start[l] + counts[l])] = l
    r = k - start[lv]
    u = unit[lv] + ((r >> 1) << (2 * (lv - lmin)))
    x, y = morton_decode(u, mutant)
    x0, y0 = x << lmin, y << lmin
    half = r & 1
    f = order
    ro = np.zeros(F, np.int64) if mutant == "rot_ignored" else np.asarray(rot, np.int64)[f]
    chart[f, 0], chart[f, 1], chart[f, 3] = x0, y0, k
    chart[f, 2] = lv | half << 8 | np.asarray(rot, np.int64)[f] << 16
    for n in range(F):
        tri = triangle(int(lv[n]), g, int(half[n]), mutant)
        for j in range(3):
            q = (j - int(ro[n])) % 3
            uv[f[n], j, 0] = np.float32(x0[n] + tri[q, 0]) / np.float32(W)
            uv[f[n], j, 1] = np.float32(y0[n] + tri[q, 1]) / np.float32(W)
    return chart, uv


# ---------------------------------------------------------------- texels

def texels(v, t, order, rot, counts, W, g, lmin, lmax, attr=None, mutant=None):
    """-> dict(face int32 [W,W], bary float32 [W,W,2], point float32 [W,W,3], flags uint8 [W,W], tex float32 [W,W,C] or None);
    row y, column x"""
    v, t = np.asarray(v, np.float64).reshape(-1, 3), np.asarray(t, np.int64).reshape(-1, 3)
    order, rot = np.asarray(order, np.int64), np.asarray(rot, np.int64)
    F = len(t)
    start, unit, cells, _ = groups(counts, lmin, lmax)
    j, i = np.meshgrid(np.arange(W, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    m = morton_encode(i >> lmin, j >> lmin, mutant)
    lv = np.full((W, W), -1, np.int64)
    for l in range(lmax, lmin - 1, -1):
        lv[(m >= unit[l]) & (m < unit[l] + (cells[l] << (2 * (l - lmin))))] = l
    has = lv >= 0
    l0 = np.where(has, lv, lmin)
    s = np.int64(1) << l0
    il, jl = i & (s - 1), j & (s - 1)
    half = (il + jl > s - 1 - (1 if mutant == "diagonal_to_wrong_half" else 0)).astype(np.int64)
    r = (((m - unit[l0]) >> (2 * (l0 - lmin))) << 1) + half
    cnt = np.asarray(counts, np.int64)[l0]
    mapped = has & (r < cnt)
    if mutant == "odd_tail_mapped":
        mapped, r = has & (cnt > 0), np.minimum(r, cnt - 1)
    face = np.full((W, W), -1, np.int64)
    if F:
        face[mapped] = order[(start[l0] + r)[mapped]]
    face[(face < 0) | (face >= F)] = -1
    own = face >= 0
    f0 = np.where(own, face, 0)
    e = s - (3 * g + 1) - (1 if mutant == "leg_off_by_one" else 0)
    hg = (1 - half) if mutant == "halves_swapped" else half
    hx = np.where(hg == 1, 2 * (s - g) - (2 * il + 1), (2 * il + 1) - 2 * g)
    hy = np.where(hg == 1, 2 * (s - g) - (2 * jl + 1), (2 * jl + 1) - 2 * g)
    with np.errstate(all="ignore"):
        beta = hx.astype(np.float64) / (2 * e).astype(np.float64)
        gamma = hy.astype(np.float64) / (2 * e).astype(np.float64)
        if mutant == "clamped_barycentrics":
            beta, gamma = np.clip(beta, 0.0, 1.0), np.clip(gamma, 0.0, 1.0)
        flags = ((hx >= 0) & (hy >= 0) & (hx + hy <= 2 * e) & own).astype(np.uint8)
        bf, gf = beta.astype(np.float32), gamma.astype(np.float32)
        bary = np.where(own[..., None], np.stack([bf, gf], -1), np.float32(0)).astype(np.float32)
        ro = np.zeros((W, W), np.int64) if (mutant == "rot_ignored" or not F) else rot[f0]
        tri = t[f0] if F else np.zeros((W, W, 3), np.int64)
        ok = ((tri >= 0) & (tri < len(v))).all(-1)
        tri = np.where(ok[..., None], tri, 0)
        ids = [np.take_along_axis(tri, ((ro + q) % 3)[..., None], -1)[..., 0] for q in range(3)]
        vv = v if len(v) else np.zeros((1, 3))
        va, vb, vc = (vv[x] for x in ids)
        pt = ((va + beta[..., None] * (vb - va)) + gamma[..., None] * (vc - va)).astype(np.float32)
        pt = np.where(ok[..., None], pt, np.float32(np.nan))
        point = np.where(own[..., None], pt, np.float32(0)).astype(np.float32)
        tex = None
        if attr is not None:
            attr = np.asarray(attr, np.float32)
            wa = (np.float32(1) - bf) - gf
            xa, xb, xc = (attr[x] for x in ids)
            tx = (wa[..., None] * xa + bf[..., None] * xb) + gf[..., None] * xc
            tx = np.where(ok[..., None], tx, np.float32(np.nan))
            tex = np.where(own[..., None], tx, np.float32(0)).astype(np.float32)
    return dict(face=face.astype(np.int32), bary=bary, point=point, flags=flags, tex=tex)


# ---------------------------------------------------------------- sample

def sample_coords(uv, W, qface, qbary):
    """-> (live, x, y) in binary64: the continuous texel coordinates of the queries"""
    uv, qface, qbary = np.asarray(uv, np.float32), np.asarray(qface, np.int64), np.asarray(qbary, np.float64).reshape(-1, 2)
    live = (qface >= 0) & (qface < len(uv))
    c = uv[np.where(live, qface, 0)].astype(np.float64) if len(uv) else np.zeros((len(qface), 3, 2))
    with np.errstate(all="ignore"):
        bu, bv = qbary[:, 0], qbary[:, 1]
        w0 = (1.0 - bu) - bv
        u = (w0 * c[:, 0, 0] + bu * c[:, 1, 0]) + bv * c[:, 2, 0]
        vv = (w0 * c[:, 0, 1] + bu * c[:, 1, 1]) + bv * c[:, 2, 1]
        x, y = u * np.float64(W) - 0.5, vv * np.float64(W) - 0.5
    live = live & np.isfinite(x) & np.isfinite(y)
    return live, np.where(live, x, 0.0), np.where(live, y, 0.0)


def sample(uv, W, tex, qface, qbary, mutant=None):
    """-> float32 [n, C]"""
    tex = np.asarray(tex, np.float32).reshape(W, W, -1)
    live, x, y = sample_coords(uv, W, qface, qbary)
    if mutant == "half_texel_dropped":
        x, y = x + 0.5, y + 0.5
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf).astype(np.float32), (y - yf).astype(np.float32)
    if mutant == "weights_wrong_axis":
        fx, fy = fy, fx
    ix, iy = np.clip(xf, -1, W).astype(np.int64), np.clip(yf, -1, W).astype(np.int64)
    i0, i1, j0, j1 = (np.clip(q, 0, W - 1) for q in (ix, ix + 1, iy, iy + 1))
    gx, gy = (np.float32(1) - fx)[:, None], (np.float32(1) - fy)[:, None]
    fx, fy = fx[:, None], fy[:, None]
    with np.errstate(all="ignore"):
        out = (tex[j0, i0] * gx + tex[j0, i1] * fx) * gy + (tex[j1, i0] * gx + tex[j1, i1] * fx) * fy
    return np.where(live[:, None], out, np.float32(0)).astype(np.float32)


def build(v, t, W, g, rho, lmin=None, lmax=None, attr=None, mutant=None):
    """the whole chain at the density rho -> dict (the layout must fit)"""
    lmin = low_level(g) if lmin is None else lmin
    lmax = W.bit_length() - 1 if lmax is None else lmax
    rho2 = np.float64(rho) * np.float64(rho)
    level, rot, hist = levels(v, t, g, lmin, lmax, rho2 * rho2, mutant)
    order = sort_order(level, lmax, mutant)
    a = dict(W=W, g=g, lmin=lmin, lmax=lmax, level=level, rot=rot, hist=hist, order=order, fits=fits(hist, W, lmin, lmax))
    if a["fits"]:
        a["chart"], a["uv"] = charts(order, level, rot, hist, W, g, lmin, lmax, mutant)
        a.update(texels(v, t, order, rot, hist, W, g, lmin, lmax, attr, mutant))
    return a


# ---------------------------------------------------------------- checks: brute force from the definitions

def check_levels(v, t, a, rho):
    """level and rot of every face from the definition, face by face"""
    g, lmin, lmax = a["g"], a["lmin"], a["lmax"]
    v = np.asarray(v, np.float64)
    rho4 = (np.float64(rho) * np.float64(rho)) * (np.float64(rho) * np.float64(rho))
    for f, tri in enumerate(np.asarray(t, np.int64)):
        if ((tri < 0) | (tri >= len(v))).any():
            assert a["level"][f] == lmin and a["rot"][f] == 0, f
            continue
        p = v[tri]
        with np.errstate(all="ignore"):
            e1, e2 = p[1] - p[0], p[2] - p[0]
            n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            c2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
            want = lmin
            if np.isfinite(c2):
                want = lmax
                for l in range(lmin, lmax + 1):
                    side = np.float64(((1 << l) - 3 * g - 1) ** 2)
                    if side * side >= c2 * rho4:
                        want = l
                        break
            assert a["level"][f] == want, (f, a["level"][f], want)
            d = [((q * q)[0] + (q * q)[1]) + (q * q)[2] for q in (p[2] - p[1], p[2] - p[0], p[1] - p[0])]
            if np.all(np.isfinite(d)):
                assert d[a["rot"][f]] == max(d) and not any(d[k] == max(d) for k in range(a["rot"][f])), (f, d, a["rot"][f])
    assert np.array_equal(a["hist"], np.bincount(a["level"], minlength=NL))


def cells_of(a):
    """per face (x0, y0, side, half) from its chart"""
    c = np.asarray(a["chart"], np.int64)
    return c[:, 0], c[:, 1], np.int64(1) << (c[:, 2] & 255), (c[:, 2] >> 8) & 1


def check_layout(v, t, a):
    """cells aligned to their side, inside the square, pairwise disjoint (two faces share a cell only as its two halves);
    larger cells first and face ids ascending within a level; the UV triangle of every face is its half's triangle with the
    longest edge of the face on the hypotenuse and the orientation kept"""
    W, g = a["W"], a["g"]
    F = len(a["order"])
    x0, y0, s, half = cells_of(a)
    level = np.asarray(a["chart"], np.int64)[:, 2] & 255
    assert np.array_equal(level, a["level"])
    assert ((x0 % s == 0) & (y0 % s == 0) & (x0 >= 0) & (y0 >= 0) & (x0 + s <= W) & (y0 + s <= W)).all()
    occupied = np.zeros((W, W), np.int32)
    seen = {}
    for f in range(F):
        key = (int(x0[f]), int(y0[f]), int(s[f]))
        seen.setdefault(key, []).append(int(half[f]))
    for (x, y, side), halves in seen.items():
        assert sorted(halves) == list(range(len(halves))) and len(halves) <= 2, (x, y, side, halves)
        occupied[y:y + side, x:x + side] += 1
    assert occupied.max(initial=0) <= 1, "two cells overlap"
    rank = np.asarray(a["chart"], np.int64)[:, 3]
    assert np.array_equal(np.sort(rank), np.arange(F)) and np.array_equal(np.asarray(a["order"])[rank], np.arange(F))
    by_rank = np.argsort(rank)
    key = [(-int(level[f]), int(f)) for f in by_rank]
    assert key == sorted(key), "larger cells first, face id within a level"
    # Z-order: the units of consecutive ranks never decrease, a pair shares its cell
    unit = [interleave(int(x0[f]) >> a["lmin"], int(y0[f]) >> a["lmin"]) for f in by_rank]
    assert all(p <= q for p, q in zip(unit, unit[1:])), "cells in Z-order"
    v, t = np.asarray(v, np.float64), np.asarray(t, np.int64)
    uvt = np.asarray(a["uv"], np.float64) * W
    assert np.array_equal(uvt, np.round(uvt)), "UVs are whole texels"
    for f in range(F):
        loc = uvt[f] - [x0[f], y0[f]]
        e = int(s[f]) - (3 * g + 1)
        want = np.array([[g, g], [g + e, g], [g, g + e]], float)
        if half[f]:
            want = s[f] - want
        assert sorted(map(tuple, loc)) == sorted(map(tuple, want)), (f, loc, want)
        e1, e2 = loc[1] - loc[0], loc[2] - loc[0]
        assert e1[0] * e2[1] - e1[1] * e2[0] > 0, "orientation kept"
        if ((t[f] >= 0) & (t[f] < len(v))).all():
            p = v[t[f]]
            with np.errstate(all="ignore"):
                d3 = [((q * q)[0] + (q * q)[1]) + (q * q)[2] for q in (p[2] - p[1], p[2] - p[0], p[1] - p[0])]
            d2 = [float(((loc[(k + 2) % 3] - loc[(k + 1) % 3]) ** 2).sum()) for k in range(3)]
            if np.all(np.isfinite(d3)):
                k = int(np.argmax(d2))                                     # the corner opposite the hypotenuse
                assert d3[k] == max(d3), (f, "the longest edge is not the hypotenuse", d3, d2)


def brute_texel_owner(a):
    """face [W, W] by the loop "which cell and half contains me" over the charts"""
    W = a["W"]
    x0, y0, s, half = cells_of(a)
    face = np.full((W, W), -1, np.int32)
    for f in range(len(x0)):
        ii, jj = np.meshgrid(np.arange(s[f]), np.arange(s[f]), indexing="xy")
        mine = (ii + jj > s[f] - 1) == bool(half[f])
        block = face[y0[f]:y0[f] + s[f], x0[f]:x0[f] + s[f]]
        assert (block[mine] == -1).all(), "two faces own one texel"
        block[mine] = f
    return face


def check_texels(v, t, a):
    """the texel -> face map against the brute force; per owned texel the barycentrics reproduce the texel centre from the
    face's UVs exactly (affine, not clamped), `inside` is the exact point-in-triangle test and the world point is the same
    affine combination of the face's vertices"""
    W = a["W"]
    assert np.array_equal(a["face"], brute_texel_owner(a)), "texel -> face"
    v, t = np.asarray(v, np.float64), np.asarray(t, np.int64)
    own = a["face"] >= 0
    jj, ii = np.nonzero(own)
    f = a["face"][own].astype(np.int64)
    uvt = np.asarray(a["uv"], np.float64)[f] * W                              # [n, 3, 2], exact
    centre = np.stack([ii + 0.5, jj + 0.5], -1)
    # barycentrics of the centre in the ORIGINAL corner order, from the UVs alone (small dyadic numbers: exact up to the division)
    e1, e2, d = uvt[:, 1] - uvt[:, 0], uvt[:, 2] - uvt[:, 0], centre - uvt[:, 0]
    det = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    w1 = (d[:, 0] * e2[:, 1] - d[:, 1] * e2[:, 0]) / det
    w2 = (e1[:, 0] * d[:, 1] - e1[:, 1] * d[:, 0]) / det
    w = np.stack([1.0 - w1 - w2, w1, w2], -1)
    # (the test itself in integers: twice the centre against whole-texel corners)
    c2, q = np.stack([2 * ii + 1, 2 * jj + 1], -1), np.round(uvt).astype(np.int64)
    k1, k2, dd = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0], c2 - 2 * q[:, 0]
    idet = k1[:, 0] * k2[:, 1] - k1[:, 1] * k2[:, 0]
    m1, m2 = (dd[:, 0] * k2[:, 1] - dd[:, 1] * k2[:, 0]) * np.sign(idet), (k1[:, 0] * dd[:, 1] - k1[:, 1] * dd[:, 0]) * np.sign(idet)
    inside = (m1 >= 0) & (m2 >= 0) & (m1 + m2 <= 2 * np.abs(idet))
    assert np.array_equal(a["flags"][own] & 1, inside.astype(np.uint8)), "inside flag"
    assert not (a["flags"][~own]).any()
    ro = np.asarray(a["rot"], np.int64)[f]
    n = np.arange(len(f))
    want = np.stack([w[n, (ro + 1) % 3], w[n, (ro + 2) % 3]], -1)
    got = a["bary"][own].astype(np.float64)
    assert np.abs(got - want).max(initial=0) <= 2.0 ** -24 * np.abs(want).max(initial=1), "barycentrics (rotated b, c), unclamped"
    ok = ((t[f] >= 0) & (t[f] < len(v))).all(-1) if len(f) else np.zeros(0, bool)
    with np.errstate(all="ignore"):
        p = v[np.where(ok[:, None], t[f], 0)] if len(v) else np.zeros((len(f), 3, 3))
        ref = (w[:, :, None] * p).sum(1)
        scale = (np.abs(w)[:, :, None] * np.abs(p)).sum(1)
        err = np.abs(a["point"][own].astype(np.float64) - ref)
    fin = ok[:, None] & np.isfinite(ref) & (scale < 1e38)                   # (beyond it binary32 overflows)
    assert (err[fin] <= 4 * 2.0 ** -24 * scale[fin] + 1e-300).all(), "world point"
    assert np.isnan(a["point"][own][~ok]).all()
    return w, (jj, ii, f)


def surface_queries(t, rng, n_random=64):
    """(face, bary [.., 2]) of n_random random points plus the corners and edge midpoints of every face"""
    F = len(t)
    fixed = np.array([[0, 0], [1, 0], [0, 1], [.5, 0], [0, .5], [.5, .5]], np.float64)
    r = rng.random((F, n_random, 2))
    flip = r.sum(-1) > 1
    r[flip] = 1 - r[flip]
    b = np.concatenate([np.broadcast_to(fixed, (F, 6, 2)), r], 1)
    return np.repeat(np.arange(F, dtype=np.int32), b.shape[1]), b.reshape(-1, 2)


def end_to_end(v, t, a, attr, qface, qbary, got):
    """the worst ratio |got - interpolation| / (2^-24 absref) over the queries: `got` = sample(a, tex) [n, C] against the
    barycentric interpolation of attr in binary64; absref from the texels' own affine weights"""
    W = a["W"]
    t, attr = np.asarray(t, np.int64), np.asarray(attr, np.float64)
    w, (jj, ii, f) = check_texels(v, t, a)
    absw = np.zeros((W, W, attr.shape[1]))
    absw[jj, ii] = (np.abs(w)[:, :, None] * np.abs(attr[t[f]])).sum(1)
    live, x, y = sample_coords(a["uv"], W, qface, qbary)
    assert live.all()
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf)[:, None], (y - yf)[:, None]
    i0, j0 = xf.astype(np.int64), yf.astype(np.int64)
    # the footprint property at work: the four texels belong to the query's face (or carry weight zero)
    for di, dj, wt in ((0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)):
        inb = (i0 + di >= 0) & (i0 + di < W) & (j0 + dj >= 0) & (j0 + dj < W)
        assert inb.all(), "a lookup leaves the square"
        assert (a["face"][j0 + dj, i0 + di] == qface).all(), "a lookup touches a texel of another face"
    absref = (absw[j0, i0] * (1 - fx) + absw[j0, i0 + 1] * fx) * (1 - fy) + (absw[j0 + 1, i0] * (1 - fx) + absw[j0 + 1, i0 + 1] * fx) * fy
    bu, bv = qbary[:, 0:1], qbary[:, 1:2]
    tri = t[qface]
    ref = (1 - bu - bv) * attr[tri[:, 0]] + bu * attr[tri[:, 1]] + bv * attr[tri[:, 2]]
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert (err[absref == 0] == 0).all()
    return float((err[absref > 0] / (2.0 ** -24 * absref[absref > 0])).max(initial=0.0))


# ---------------------------------------------------------------- cases

def cube():
    v = np.array([[x, y, z] for x in (0., 1.) for y in (0., 1.) for z in (0., 1.)])
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = np.array([tri for a, b, c, d in q for tri in ((a, b, c), (a, c, d))], np.int64)
    return v, t


def level_span(g, lmin, lmax, rho=1.0, seed=3):
    """a mesh of separate triangles whose areas hit every level from lmin to lmax at the density rho, with odd counts in
    several levels, in scrambled order and with all three edges taking the longest's place"""
    rng = np.random.default_rng(seed)
    v, t = [], []
    for n, l in enumerate(range(lmin, lmax + 1)):
        for k in range((3, 1, 5, 3)[n % 4] if l < lmax else 1):
            side = (leg(l, g) - 0.5) / rho if l > lmin else 0.5 * leg(lmin, g) / rho
            o = rng.normal(size=3) * 3
            p = [o, o + [side, 0, 0], o + [0.2 * side, 0, side]]           # |e1 x e2| = side^2: just under leg(l)^2 rho^-2
            s = (n + k) % 3
            base = len(v)
            v += p[s:] + p[:s]
            t.append((base, base + 1, base + 2))
    t = np.array(t, np.int64)[rng.permutation(len(t))]
    return np.array(v), t


def odd_faces():
    """degenerate, coincident and NaN faces, faces with a bad vertex id, and equal longest edges (ties of rot)"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [np.nan, 0, 0], [1e200, 0, 0], [0, 1e200, 0], [1, 1, 0], [0, 0, 1.],
                  [0.5, 2, 0]])
    t = np.array([[0, 1, 2], [0, 1, 3], [0, 0, 0], [0, 1, 2], [0, 1, 4], [0, 5, 6], [1, 2, 0], [2, 0, 1], [0, 1, 10], [-1, 1, 2],
                  [1, 2, 8], [0, 1, 9], [1, 9, 0], [9, 0, 1]], np.int64)
    return v, t


def far_faces():
    v, t = cube()
    return v * 0.37 + np.array([1000.0, -1000.0, 1000.0]), t


def attributes(n_vertices, channels=12, seed=5):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n_vertices, channels)).astype(np.float32)
    a[:, 0] = 1.0                                                            # (a constant channel: any weights that sum to 1)
    return a
