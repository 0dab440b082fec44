"""Restatement of the ray caster (esr_nerf_amd/csrc/bvh.hip, raycast.py, sources.source_visibility) in numpy float64 and
Python integers: section T of include/esr_hip.h taken word by word, with none of the kernels' machinery.

  brute            rays x faces by brute force: the nearest hit (ties to the smaller id), the any-hit answer, and the
                   AMBIGUOUS rays with their acceptable answers, by the project's two constants (raster_ref.BAND, KEY_RES):
                     some face with t in range has a barycentric with |b| < BAND, or
                     the two nearest hits lie within KEY_RES relative of each other, or a hit of t_min / t_max.
                   The per-face arithmetic IS the binary64 emulation of the kernel's order of operations (numpy rounds
                   every operation on its own), so the GPU's t, u, v are compared with it bit for bit
  t_reference      t in extended precision and `absref`, the sum of the absolute values of the terms of t's numerator over |det|
  keys             the Morton keys, the cells in Python integers
  radix_tree       the tree BY ITS DEFINITION: a range of sorted (key, position) strings splits where their highest differing
                   bit changes; built top-down, no search of Karras's
  boxes            the outward-rounded binary32 boxes of faces and nodes
  walk             a Python walk of that tree, and its mutants
  source_samples   the sample-point rule of sources.source_visibility

The bound on t: |t - t_ref| <= K_T 2^-53 absref.  K_T is the next power of two above the worst ratio the GPU tests and the
binary64 emulation show over all their cases (the two are the same numbers: the GPU's t is bit-equal to the emulation).
"""
import numpy as np

from raster_ref import BAND, KEY_RES, generic_cam, inside_cam, lumpy_sphere, pixel_rays  # noqa: F401

U = 2.0 ** -53
K_T = 8.0
K_T_WORST = 4.71         # the worst |t - t_ref| / (2^-53 absref) over every case of the CPU and GPU tests: 4.707 on twins/random (-s prints them)
CELLS = 1 << 21
KEY_NONE = (1 << 63) - 1


# ----------------------------------------------------------------------------------------------------------------------
# the triangle test in the kernel's order of operations


def intersect(o, d, v, tr):
    """rays (o, d [N, 3]) x faces -> dict of [N, F] arrays t, u, v, w, det and absref_num (the sum of the absolute values of
    the six products of t's numerator); every operation a separately rounded binary64 one, in the order of the header"""
    v = np.asarray(v, np.float64)
    tr = np.asarray(tr, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        a = v[tr[:, 0]][None]
        e1 = (v[tr[:, 1]] - v[tr[:, 0]])[None]
        e2 = (v[tr[:, 2]] - v[tr[:, 0]])[None]
        o, d = o[:, None, :], d[:, None, :]
        s = o - a
        px = d[..., 1] * e2[..., 2] - d[..., 2] * e2[..., 1]
        py = d[..., 2] * e2[..., 0] - d[..., 0] * e2[..., 2]
        pz = d[..., 0] * e2[..., 1] - d[..., 1] * e2[..., 0]
        det = (e1[..., 0] * px + e1[..., 1] * py) + e1[..., 2] * pz
        qx = s[..., 1] * e1[..., 2] - s[..., 2] * e1[..., 1]
        qy = s[..., 2] * e1[..., 0] - s[..., 0] * e1[..., 2]
        qz = s[..., 0] * e1[..., 1] - s[..., 1] * e1[..., 0]
        ok = (det != 0.0) & np.isfinite(det)
        dd = np.where(ok, det, np.nan)
        u = ((s[..., 0] * px + s[..., 1] * py) + s[..., 2] * pz) / dd
        w_ = ((d[..., 0] * qx + d[..., 1] * qy) + d[..., 2] * qz) / dd
        t = ((e2[..., 0] * qx + e2[..., 1] * qy) + e2[..., 2] * qz) / dd
        num = (np.abs(e2[..., 0]) * (np.abs(s[..., 1] * e1[..., 2]) + np.abs(s[..., 2] * e1[..., 1])) +
               np.abs(e2[..., 1]) * (np.abs(s[..., 2] * e1[..., 0]) + np.abs(s[..., 0] * e1[..., 2])) +
               np.abs(e2[..., 2]) * (np.abs(s[..., 0] * e1[..., 1]) + np.abs(s[..., 1] * e1[..., 0])))
        return dict(t=t, u=u, v=w_, w=(1.0 - u) - w_, det=dd, absref=num / np.abs(dd))


def t_reference(o, d, v, tr, face):
    """t of ray k against face[k] in extended precision (the plane's equation, not the kernel's expression)"""
    L = np.longdouble
    a, b, c = (np.asarray(v)[np.asarray(tr)[face, k]].astype(L) for k in range(3))
    n = np.cross(b - a, c - a)
    return ((a - o.astype(L)) * n).sum(-1) / (d.astype(L) * n).sum(-1)


def brute(v, tr, o, d, t_min=0.0, t_max=np.inf, skip=None, chunk=1 << 21):
    """-> dict: face int64 [N] (-1), t, u, v float64 [N] (the emulation's values; t = inf, u = v = 0 for none), hit bool [N],
    absref [N], ambiguous bool [N], accept {ray: (set of faces, empty_ok)}"""
    v = np.asarray(v, np.float64)
    tr = np.asarray(tr, np.int64).reshape(-1, 3)
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    N, F = len(o), len(tr)
    lo = np.broadcast_to(np.asarray(t_min, np.float64), (N,))
    hi = np.broadcast_to(np.asarray(t_max, np.float64), (N,))
    sk = np.full(N, -1, np.int64) if skip is None else np.asarray(skip, np.int64)
    out = dict(face=np.full(N, -1, np.int64), t=np.full(N, np.inf), u=np.zeros(N), v=np.zeros(N), absref=np.zeros(N),
               ambiguous=np.zeros(N, bool), accept={})
    step = max(1, chunk // max(F, 1))
    ids = np.arange(F)
    with np.errstate(all="ignore"):
        fin = (np.isfinite(o).all(1) & np.isfinite(d).all(1))
        for r0 in range(0, N, step):
            sl = slice(r0, min(r0 + step, N))
            if F == 0:
                continue
            x = intersect(o[sl], d[sl], v, tr)
            t, bmin = x["t"], np.minimum(np.minimum(x["u"], x["v"]), x["w"])
            babs = np.minimum(np.minimum(np.abs(x["u"]), np.abs(x["v"])), np.abs(x["w"]))
            live = (ids[None, :] != sk[sl, None]) & fin[sl, None]
            l, h = lo[sl, None], hi[sl, None]
            inr = live & (t > l) & (t <= h)
            hit = inr & (bmin >= 0)
            th = np.where(hit, t, np.inf)
            k = np.argmin(th, 1)                                   # (the first of equal values: the smallest id)
            rows = np.arange(th.shape[0])
            t1 = th[rows, k]
            got = np.isfinite(t1) | hit[rows, k]
            th2 = th.copy()
            th2[rows, k] = np.inf
            t2 = th2.min(1)
            # what a legitimate other answer could turn on: a barycentric near 0 of a face near the interval, two hits
            # that the constant cannot tell apart, a hit (or near hit) at an end of the interval
            tol = KEY_RES * np.maximum(x["absref"], np.maximum(np.abs(l), np.where(np.isfinite(h), np.abs(h), 0.0)))
            near_r = live & (t > l - tol) & (t <= h + tol)
            band = (near_r & (babs < BAND)).any(1)
            maybe = near_r & (bmin >= -BAND)
            ends = (maybe & ((np.abs(t - l) <= tol) | (np.abs(t - h) <= tol))).any(1)
            amb = band | ends | (np.isfinite(t2) & (t2 - t1 <= KEY_RES * np.abs(t1)))
            sure = inr & (bmin >= BAND) & (t > l + tol) & (t <= h - tol)
            sure_t = np.where(sure, t, np.inf).min(1)
            for r in np.flatnonzero(amb):
                ok = maybe[r] & (t[r] <= sure_t[r] + KEY_RES * np.abs(sure_t[r]) if np.isfinite(sure_t[r]) else maybe[r])
                out["accept"][r0 + int(r)] = (set(int(f) for f in np.flatnonzero(ok)), not np.isfinite(sure_t[r]))
            out["ambiguous"][sl] = amb
            out["face"][sl] = np.where(got, k, -1)
            for name in ("t", "u", "v", "absref"):
                out[name][sl] = np.where(got, x[name][rows, k], out[name][sl])
    out["hit"] = out["face"] >= 0
    return out


def t_ratio(v, tr, o, d, ref, face=None, t=None):
    """the worst |t - t_ref| / (2^-53 absref) over the rays whose face equals the brute force's (t: the values under test,
    default the emulation's own)"""
    face = ref["face"] if face is None else np.asarray(face, np.int64)
    t = ref["t"] if t is None else np.asarray(t, np.float64)
    same = (face == ref["face"]) & (face >= 0)
    if not same.any():
        return 0.0
    tref = t_reference(o[same], d[same], v, tr, face[same])
    err = np.abs(t[same].astype(np.longdouble) - tref).astype(np.float64)
    return float((err / (U * ref["absref"][same])).max())


def check_hits(ref, face, t, bary, what=""):
    """the nearest-hit checks of one case against ``brute``'s dict; returns the ambiguous share"""
    face, t, bary = np.asarray(face, np.int64), np.asarray(t, np.float64), np.asarray(bary, np.float64).reshape(-1, 2)
    clear = ~ref["ambiguous"]
    bad = np.flatnonzero(clear & (face != ref["face"]))
    assert len(bad) == 0, (what, "face differs on unambiguous rays", bad[:8], face[bad[:8]], ref["face"][bad[:8]])
    for r in np.flatnonzero(ref["ambiguous"]):
        faces, empty_ok = ref["accept"][int(r)]
        assert (face[r] in faces) or (face[r] == -1 and empty_ok), (what, "ambiguous ray outside its set", int(r), int(face[r]), faces)
    assert np.array_equal(np.isposinf(t), face == -1), (what, "t is +inf exactly where there is no face")
    return float(ref["ambiguous"].mean()) if len(face) else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# the build


def scene_box(v):
    v = np.asarray(v, np.float64).reshape(-1, 3)
    ok = np.isfinite(v).all(1)
    if not ok.any():
        return np.array([np.inf] * 3 + [-np.inf] * 3)
    return np.concatenate([v[ok].min(0), v[ok].max(0)])


def round_out(lo, hi):
    """binary32 lo rounded down, hi rounded up"""
    with np.errstate(over="ignore"):
        l, h = lo.astype(np.float32), hi.astype(np.float32)
    l = np.where(l.astype(np.float64) > lo, np.nextafter(l, np.float32(-np.inf)), l)
    h = np.where(h.astype(np.float64) < hi, np.nextafter(h, np.float32(np.inf)), h)
    return l.astype(np.float32), h.astype(np.float32)


def keys(v, tr, nearest=False):
    """-> (keys int64 [F], boxes float32 [F, 6]); ``nearest``: the mutant that rounds the boxes to nearest"""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    tr = np.asarray(tr, np.int64).reshape(-1, 3)
    sb = scene_box(v)
    out_k, out_b = np.zeros(len(tr), np.int64), np.zeros((len(tr), 6), np.float32)
    for f, ids in enumerate(tr):
        p = v[ids] if ((ids >= 0) & (ids < len(v))).all() else np.full((3, 3), np.nan)
        if not np.isfinite(p).all():
            out_k[f] = KEY_NONE
            out_b[f] = [np.inf] * 3 + [-np.inf] * 3
            continue
        lo, hi = p.min(0), p.max(0)
        key = 0
        for a in range(3):
            c = np.float64(0.5) * lo[a] + np.float64(0.5) * hi[a]
            ext = sb[3 + a] - sb[a]
            cell = int(np.floor(((c - sb[a]) / ext) * np.float64(CELLS))) if ext > 0 else 0
            cell = min(max(cell, 0), CELLS - 1)
            for k in range(21):
                key |= ((cell >> k) & 1) << (3 * k + 2 - a)
        out_k[f] = key
        if nearest:
            out_b[f] = np.concatenate([lo.astype(np.float32), hi.astype(np.float32)])
        else:
            out_b[f] = np.concatenate(round_out(lo, hi))
    return out_k, out_b


class Tree:
    """order int64 [F]; skeys; child int32 [F - 1, 2] (>= 0 node, < 0 ~face); parent int32 [F - 1] (2 p + side, -1 root);
    leaf_parent int32 [F]; depth (levels of internal nodes above the deepest leaf)"""


def radix_tree(k):
    """the tree by the definition, top-down over the sorted (key, position) strings"""
    k = np.asarray(k, np.int64)
    n = len(k)
    T = Tree()
    T.order = np.argsort(k, kind="stable").astype(np.int64)
    T.skeys = k[T.order]
    T.child = np.zeros((max(n - 1, 0), 2), np.int32)
    T.parent = np.full(max(n - 1, 0), -1, np.int32)
    T.leaf_parent = np.full(n, -1, np.int32)
    T.depth = 0
    if n < 2:
        return T
    s = [(int(T.skeys[i]) << 32) | i for i in range(n)]
    todo = [(0, n - 1, 0, 0)]                                       # first, last, the node's index, its depth
    while todo:
        first, last, idx, depth = todo.pop()
        T.depth = max(T.depth, depth + 1)
        top = (s[first] ^ s[last]).bit_length() - 1               # the highest differing bit of the range
        g = first
        while not (s[g + 1] >> top) & 1:                           # the last string with that bit clear
            g += 1
        for side, (a, b, ci) in enumerate(((first, g, g), (g + 1, last, g + 1))):
            if a == b:
                T.child[idx, side] = ~int(T.order[a])
                T.leaf_parent[a] = 2 * idx + side
            else:
                T.child[idx, side] = ci
                T.parent[ci] = 2 * idx + side
                todo.append((a, b, ci, depth + 1))
    return T


def trie_tree(k):
    """a second, independent construction: the compressed binary trie of the sorted strings, built by inserting them one
    by one -> the set of (first, last) ranges of its internal nodes with their split positions"""
    k = np.asarray(k, np.int64)
    order = np.argsort(k, kind="stable")
    s = [format((int(k[f]) << 32) | i, "095b") for i, f in enumerate(order)]
    root = {}
    for i, w in enumerate(s):
        node = root
        for ch in w:
            node = node.setdefault(ch, {})
        node["leaf"] = i
    ranges = set()

    def span(node):
        if "leaf" in node:
            return node["leaf"], node["leaf"]
        kids = [span(node[c]) for c in "01" if c in node]
        if len(kids) == 2:
            ranges.add((kids[0][0], kids[1][1], kids[0][1]))
        return kids[0][0], kids[-1][1]
    import sys
    sys.setrecursionlimit(10000)
    if s:
        span(root)
    return ranges


def tree_ranges(T):
    """(first, last, split) of every internal node of a Tree, from its links alone"""
    n = len(T.order)
    pos_of = {int(f): i for i, f in enumerate(T.order)}
    out = {}

    def span(link):
        if link < 0:
            return pos_of[~link], pos_of[~link]
        a, b = span(int(T.child[link, 0])), span(int(T.child[link, 1]))
        out[link] = (a[0], b[1], a[1])
        return a[0], b[1]
    import sys
    sys.setrecursionlimit(10000)
    if n >= 2:
        span(0)
    return out


def boxes(T, face_boxes):
    """node boxes float32 [F - 1, 2, 6] (the boxes of each node's two children) and the root's box [6]"""
    n = len(T.order)
    nb = np.zeros((max(n - 1, 0), 2, 6), np.float32)
    if n == 0:
        return nb, np.array([np.inf] * 3 + [-np.inf] * 3, np.float32)
    if n == 1:
        return nb, face_boxes[T.order[0]].copy()
    import sys
    sys.setrecursionlimit(10000)

    def fit(link):
        if link < 0:
            return face_boxes[~link]
        for side in range(2):
            nb[link, side] = fit(int(T.child[link, side]))
        return np.concatenate([np.minimum(nb[link, 0, :3], nb[link, 1, :3]), np.maximum(nb[link, 0, 3:], nb[link, 1, 3:])])
    return nb, fit(0)


def node_words(T, nb):
    """the esr_bvh_node_t records as int32 [F - 1, 16]"""
    n = len(T.child)
    w = np.zeros((n, 16), np.int32)
    w[:, :12] = nb.reshape(n, 12).view(np.int32)
    w[:, 12:14], w[:, 14] = T.child, T.parent
    return w


# ----------------------------------------------------------------------------------------------------------------------
# a walk of the restated tree (plain Python, one ray at a time) and its mutants

MUTANTS = ("exclusive_prune", "larger_id_on_ties", "t_min_inclusive", "cull_backfaces", "ignore_skip", "nearest_boxes",
           "zero_slab", "no_eps")


def _slab(o, d, b, t0, t1, mutant):
    lo, hi = t0, t1
    for a in range(3):
        bl, bh = float(b[a]), float(b[3 + a])
        if bl > bh:
            return None
        da = d[a]
        if da == 0.0:
            if mutant == "zero_slab":
                da = 1e-6                                           # (the perturbed direction of esr_ray_trange)
            else:
                if not bl <= o[a] <= bh:
                    return None
                continue
        x, y = (bl - o[a]) / da, (bh - o[a]) / da
        lo, hi = max(lo, min(x, y)), min(hi, max(x, y))
    if (lo < hi) if mutant == "exclusive_prune" else (lo <= hi):
        return lo
    return None


def _tri(o, d, p, t_min, t_max, mutant):
    """the header's triangle test on Python floats (binary64, every operation rounded on its own, the same order)"""
    (a0, a1, a2), b, c = (float(x) for x in p[0]), p[1], p[2]
    e10, e11, e12 = float(b[0]) - a0, float(b[1]) - a1, float(b[2]) - a2
    e20, e21, e22 = float(c[0]) - a0, float(c[1]) - a1, float(c[2]) - a2
    o0, o1, o2, d0, d1, d2 = (float(x) for x in (*o, *d))
    px, py, pz = d1 * e22 - d2 * e21, d2 * e20 - d0 * e22, d0 * e21 - d1 * e20
    det = (e10 * px + e11 * py) + e12 * pz
    if det == 0.0 or det != det or abs(det) == float("inf"):
        return None
    s0, s1, s2 = o0 - a0, o1 - a1, o2 - a2
    qx, qy, qz = s1 * e12 - s2 * e11, s2 * e10 - s0 * e12, s0 * e11 - s1 * e10
    u = ((s0 * px + s1 * py) + s2 * pz) / det
    v = ((d0 * qx + d1 * qy) + d2 * qz) / det
    t = ((e20 * qx + e21 * qy) + e22 * qz) / det
    w = (1.0 - u) - v
    if not (u >= 0 and v >= 0 and w >= 0 and t <= t_max):
        return None
    if not ((t >= t_min) if mutant == "t_min_inclusive" else (t > t_min)):
        return None
    if mutant == "cull_backfaces" and det < 0:
        return None
    return t


def walk(T, nb, v, tr, o, d, t_min=0.0, t_max=np.inf, skip=-1, any_hit=False, mutant=None):
    """-> (face, t) of one ray through the restated tree: near child first, nothing pruned at equality, ties to the
    smaller id.  (A recursive walk: none of the kernel's trail.)"""
    v, tr = np.asarray(v, np.float64), np.asarray(tr, np.int64)
    best = [-1, t_max]
    if not (np.isfinite(o).all() and np.isfinite(d).all()):
        return -1, np.inf
    if mutant == "ignore_skip":
        skip = -1

    def leaf(f):
        if f == skip:
            return
        t = _tri(o, d, v[tr[f]], t_min, t_max, mutant)
        if t is None:
            return
        if best[0] < 0 or t < best[1] or (t == best[1] and ((f > best[0]) if mutant == "larger_id_on_ties" else (f < best[0]))):
            best[0], best[1] = f, t

    def visit(link):
        if any_hit and best[0] >= 0:
            return
        if link < 0:
            return leaf(~link)
        e = [_slab(o, d, nb[link, s], t_min, best[1], mutant) for s in range(2)]
        for s in ((1, 0) if e[1] is not None and (e[0] is None or e[1] < e[0]) else (0, 1)):
            if e[s] is None:
                continue
            if (e[s] < best[1]) if mutant == "exclusive_prune" else (e[s] <= best[1]):
                visit(int(T.child[link, s]))
    import sys
    sys.setrecursionlimit(10000)
    if len(tr) == 1:
        leaf(0)
    elif len(tr) > 1:
        visit(0)
    return (best[0], best[1]) if best[0] >= 0 else (-1, np.inf)


def built(v, tr, nearest=False):
    """(Tree, node boxes, face boxes, keys) of a mesh"""
    k, fb = keys(v, tr, nearest)
    T = radix_tree(k)
    nb, root = boxes(T, fb)
    T.root_box = root
    return T, nb, fb, k


# ----------------------------------------------------------------------------------------------------------------------
# meshes and rays of the cases both test files share


def few_faces(n):
    """n <= 3 faces in general position"""
    v = np.array([[0.1, 0.2, 0.0], [1.0, 0.1, 0.2], [0.2, 1.1, 0.1], [0.9, 1.0, 0.7], [0.0, 0.3, 0.9], [1.2, 0.2, 1.0]])
    return v, np.array([[0, 1, 2], [1, 3, 2], [0, 4, 5]], np.int64)[:n]


def twins(n=500):
    """2 n faces, n tilted triangles whose boxes all have their centre at the origin, each of them twice: every key is equal"""
    k = np.arange(n, dtype=np.float64)
    s, h = 0.3 + k / n, 0.05 + 0.4 * ((k * 7) % n) / n
    v = np.stack([np.stack([-s, -s, -h], 1), np.stack([s, -s, h], 1), np.stack([0 * s, s, 0 * h], 1)], 1).reshape(-1, 3)
    t = np.arange(3 * n).reshape(n, 3)
    return v, np.concatenate([t, t]).astype(np.int64)


def chain(n=80):
    """n small faces whose keys each open a new highest bit -- centres at 2^-k along x, then y, then z in turn -- and, for the
    rest of them, centres inside the first cell (equal keys): the key bits chain 63 levels deep and the position bits of the
    equal keys add to that.  (Centres at 2^-k along ONE diagonal do not get there: a step down the diagonal opens three key
    bits at once and from k = 21 on the keys are equal -- 27 levels at 80 faces, 29 at 200, by this restatement.)"""
    cs, rs = [], []
    for k in range(1, 22):
        for a in range(3):
            c = np.zeros(3)
            c[a] = 2.0 ** -k
            cs.append(c), rs.append(2.0 ** -(k + 4))
    while len(cs) < n:
        i = len(cs) - 63
        cs.append(np.array([1.0, 1.0, 1.0]) * 2.0 ** -30 * (1 + i)), rs.append(2.0 ** -32)
    v, t = [], []
    for c, r in zip(cs, rs):
        b = len(v)
        v += [c + r * np.array([0.0, 0.0, 0.0]), c + r * np.array([1.0, 0.1, 0.3]), c + r * np.array([0.2, 1.0, 0.5])]
        t.append((b, b + 1, b + 2))
    return np.array(v), np.array(t, np.int64)


def far_small():
    """two small faces a thousand units from the origin, in planes y = const: the binary32 grid is 6e-5 there, 6 % of a face,
    and 1000.001 rounds DOWN to binary32 -- a box rounded to nearest leaves a strip of the first face outside"""
    T, Y = 1000.001, 1000.0005
    assert float(np.float32(T)) < T - 2e-5
    v = np.array([[1000.0, Y, 1000.0], [T, Y, 1000.0], [T, Y, T], [1000.0, Y + 0.002, 1000.0], [T, Y + 0.002, 1000.0],
                  [1000.0, Y + 0.002, T]])
    return v, np.array([[0, 1, 2], [3, 4, 5]], np.int64)


def far_small_rays():
    """along y (two zero components) through the strip x in (float32(T), T) of the first face, and through its middle"""
    o = np.array([[1000.00099, 999.0, 1000.0005], [1000.0006, 999.0, 1000.0003], [1000.00099, 1001.0, 1000.0002]])
    return o, np.array([[0.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.0, -2.0, 0.0]])


def with_nan_vertex():
    v, t = lumpy_sphere()
    v = v.copy()
    v[5, 1] = np.nan
    return v, t


def rays_at_faces(v, tr, n, seed, radius=2.5):
    """n rays from random points of a sphere around the mesh towards random interior points of random faces"""
    rng = np.random.default_rng(seed)
    v = np.asarray(v)
    ok = np.flatnonzero(np.isfinite(v[tr]).all((1, 2)))
    f = ok[rng.integers(0, len(ok), n)]
    b = rng.dirichlet((2.0, 2.0, 2.0), n)
    target = (v[tr[f]] * b[:, :, None]).sum(1)
    centre, ext = np.nanmean(v, 0), np.nanmax(np.abs(v - np.nanmean(v, 0)))
    g = rng.normal(size=(n, 3))
    o = centre + radius * ext * g / np.linalg.norm(g, axis=1, keepdims=True)
    return o, (target - o) * rng.uniform(0.5, 2.0, (n, 1))


def axis_rays(v, tr):
    """rays with zero components in every pattern (one or two zeros, both signs) through interior points of faces, and the
    same from 1e5 away"""
    v = np.asarray(v)
    rng = np.random.default_rng(11)
    o, d = [], []
    for far in (3.0, 1e5):
        for pattern in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
            for sign in (1.0, -1.0):
                for f in rng.integers(0, len(tr), 6):
                    b = rng.dirichlet((3.0, 3.0, 3.0))
                    target = (v[tr[f]] * b[:, None]).sum(0)
                    dd = np.array(pattern, np.float64) * sign * rng.uniform(0.5, 1.5, 3)
                    o.append(target - far * dd), d.append(dd)
    return np.array(o), np.array(d)


def special_rays(v, tr):
    """rays that start on a vertex, run along an edge, or are not finite"""
    v = np.asarray(v)
    c = v.mean(0)
    o, d = [], []
    for f in (0, 17, 100):
        a, b = v[tr[f, 0]], v[tr[f, 1]]
        o += [a, a, a, a - (b - a)]
        d += [c - a, a - c, b - a, b - a]                           # from a vertex inwards / outwards, along an edge (twice)
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            oo, dd = np.array([3.0, 0.2, 0.1]), np.array([-1.0, 0.0, 0.0])
            oo[k] = bad
            o.append(oo), d.append(dd)
            oo, dd = np.array([3.0, 0.2, 0.1]), np.array([-1.0, 0.01, 0.02])
            dd[k] = bad
            o.append(oo), d.append(dd)
    return np.array(o), np.array(d)


def room():
    """A closed box room [0, 4] x [0, 3] x [0, 2.5] on an uneven grid, a slab hanging under the ceiling, and two emissive
    patches: on the ceiling above the slab and on the wall x = 0.  -> (v, tr, face_source int32 [F], n_sources)"""
    xs, ys, zs = np.array([0.0, 0.7, 1.5, 2.6, 4.0]), np.array([0.0, 0.9, 2.1, 3.0]), np.array([0.0, 1.1, 2.5])
    v, t, src = [], [], []

    def quad_grid(ax, const, us, ws, source_of=lambda i, j: -1):
        for i in range(len(us) - 1):
            for j in range(len(ws) - 1):
                q = []
                for uu, ww in ((us[i], ws[j]), (us[i + 1], ws[j]), (us[i + 1], ws[j + 1]), (us[i], ws[j + 1])):
                    p = [0.0, 0.0, 0.0]
                    p[ax], p[(ax + 1) % 3], p[(ax + 2) % 3] = const, uu, ww
                    q.append(p)
                b = len(v)
                v.extend(q)
                t.extend([(b, b + 1, b + 2), (b, b + 2, b + 3)])
                src.extend([source_of(i, j)] * 2)
    quad_grid(2, 0.0, xs, ys)                                                        # floor (z = 0): axes x, y
    quad_grid(2, 2.5, xs, ys, lambda i, j: 0 if i in (1, 2) and j == 1 else -1)     # ceiling, the patch x 0.7 .. 2.6, y 0.9 .. 2.1
    quad_grid(0, 0.0, ys, zs, lambda i, j: 1 if i == 1 else -1)                      # wall x = 0: axes y, z; the patch y 0.9 .. 2.1
    quad_grid(0, 4.0, ys, zs)
    quad_grid(1, 0.0, zs, xs)                                                        # wall y = 0: axes z, x
    quad_grid(1, 3.0, zs, xs)
    quad_grid(2, 1.9, np.array([0.9, 1.6, 2.4]), np.array([1.0, 1.4, 2.0]))          # the slab, under part of the ceiling patch
    return np.array(v, np.float64), np.array(t, np.int64), np.array(src, np.int32), 2


def room_points():
    """query points: on the floor under the slab, beside it, and outside the room"""
    return np.array([[1.63, 1.47, 0.013], [1.21, 1.71, 0.02], [3.33, 0.41, 0.017], [3.1, 2.6, 0.4], [0.31, 1.53, 1.23],
                     [5.2, 1.3, 1.1], [2.0, 1.5, 3.4], [-1.1, 1.4, 0.9]])


# ----------------------------------------------------------------------------------------------------------------------
# sources.source_visibility


def source_samples(v, tr, face_source, n_sources, samples):
    """-> (face [S][n], point [S][n, 3], margin): the rule of sources.source_samples in a direct float64 loop.  margin is the
    smallest relative distance of a threshold from a cumulative area: the choice is safe from the order of a sum when it
    is far above rounding"""
    v, tr = np.asarray(v, np.float64), np.asarray(tr, np.int64)
    faces, points, margin = [], [], np.inf
    for s in range(n_sources):
        ids = np.flatnonzero(np.asarray(face_source) == s)
        a, b, c = (v[tr[ids, k]] for k in range(3))
        e1, e2 = b - a, c - a
        n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        area = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2) * 0.5
        cum = np.cumsum(area)
        n = min(samples, len(ids))
        got = []
        for k in range(n):
            thr = ((k + 0.5) / n) * cum[-1]
            j = int(np.argmax(cum >= thr))
            margin = min(margin, float(np.abs(cum - thr).min() / cum[-1]))
            got.append(j)
        faces.append(ids[got])
        points.append(((a[got] + b[got]) + c[got]) * (1.0 / 3.0))
    return faces, points, margin


def visibility(v, tr, face_source, n_sources, pts, samples, eps=1e-6):
    """-> (share float32 [P, S], bits list per source of uint8 [P, n], ambiguous count): every segment by brute force"""
    faces, points, _ = source_samples(v, tr, face_source, n_sources, samples)
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    out = np.zeros((len(pts), n_sources), np.float32)
    bits, amb = [], 0
    for s in range(n_sources):
        n = len(faces[s])
        o = np.repeat(pts, n, 0)
        q = np.tile(points[s], (len(pts), 1))
        r = brute(v, tr, o, q - o, eps, 1.0 - eps, np.tile(faces[s], len(pts)))
        amb += int(r["ambiguous"].sum())
        occ = r["hit"].reshape(len(pts), n)
        bits.append(occ.astype(np.uint8))
        out[:, s] = ((~occ).sum(1).astype(np.float64) / n).astype(np.float32)
    return out, bits, amb


# ----------------------------------------------------------------------------------------------------------------------
# the ray cases of the nearest-hit tests: name -> dict(v, tr, o, d, t_min, t_max, skip); `generic` marks the cases whose
# ambiguous share must stay under 1 %


def camera_rays(cam):
    o, d = [], []
    for view in range(cam.n_views):
        oo, dd = pixel_rays(cam, view)
        o.append(np.broadcast_to(oo, dd.shape)), d.append(dd)
    return np.concatenate(o), np.concatenate(d)


def sphere_cases(name, v, tr):
    out = {}
    for cname, cam in (("generic_cam", generic_cam()), ("inside_cam", inside_cam())):
        o, d = camera_rays(cam)
        out[f"{name}/{cname}"] = dict(v=v, tr=tr, o=o, d=d, generic=True)
    o, d = axis_rays(v, tr)
    out[f"{name}/axis"] = dict(v=v, tr=tr, o=o, d=d)
    o, d = special_rays(v, tr)
    out[f"{name}/special"] = dict(v=v, tr=tr, o=o, d=d)
    # the interval just either side of the nearest hit, and the nearest face skipped, on the first view from outside
    oo, d = pixel_rays(generic_cam(), 0)
    o = np.broadcast_to(oo, d.shape).copy()
    base = brute(v, tr, o, d)
    got = base["face"] >= 0
    o, d, t, f = o[got], d[got], base["t"][got], base["face"][got]
    n = len(t)
    e = 1e-5
    lo = np.concatenate([np.zeros(2 * n), t * (1 - e), t * (1 + e)])
    hi = np.concatenate([t * (1 + e), t * (1 - e), np.full(2 * n, np.inf)])
    out[f"{name}/interval"] = dict(v=v, tr=tr, o=np.tile(o, (4, 1)), d=np.tile(d, (4, 1)), t_min=lo, t_max=hi)
    out[f"{name}/skip"] = dict(v=v, tr=tr, o=o, d=d, skip=f.astype(np.int32))
    return out


def other_cases(n_random):
    out = {}
    for name, (v, tr) in (("chain", chain()), ("twins", twins())):
        o, d = rays_at_faces(v, tr, n_random, seed=len(name))
        out[f"{name}/random"] = dict(v=v, tr=tr, o=o, d=d)
    v, tr = far_small()
    o, d = far_small_rays()
    out["far_small/along_y"] = dict(v=v, tr=tr, o=o, d=d)
    v, tr = with_nan_vertex()
    o, d = camera_rays(generic_cam())
    out["nan_vertex/generic_cam"] = dict(v=v, tr=tr, o=o, d=d)
    for n in (1, 2, 3):
        v, tr = few_faces(n)
        o, d = rays_at_faces(v, tr, 40, seed=n, radius=3.0)
        out[f"faces{n}/random"] = dict(v=v, tr=tr, o=o, d=d)
    return out


def room_cases():
    """axis-parallel rays inside the room (every box of a wall is flat: entry and exit distance are equal), and segments that
    end just behind a face"""
    v, tr, _, _ = room()
    pts = room_points()[:5]
    dirs = np.array([[0, 0, 1.0], [0, 0, -1.0], [1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0.3, 0.2, 1.0]])
    o, d = np.repeat(pts, len(dirs), 0), np.tile(dirs, (len(pts), 1))
    return {"room/axis": dict(v=v, tr=tr, o=o, d=d)}


def segment_case(eps=1e-4, over=5e-5):
    """segments from inside the lumpy sphere to just behind the centres of faces (the hit lies at 1 / (1 + over), between
    1 - eps and 1): not occluded -- and occluded once eps is dropped"""
    v, tr = lumpy_sphere()
    p = np.array([0.1, 0.05, -0.1])
    c = v[tr[::7]].mean(1)
    q = p + (c - p) * (1.0 + over)
    return v, tr, np.broadcast_to(p, q.shape).copy(), q, eps


def case_brute(c):
    return brute(c["v"], c["tr"], c["o"], c["d"], c.get("t_min", 0.0), c.get("t_max", np.inf), c.get("skip"))


def bary_ratio(v, tr, o, d, ref, face, u, w):
    """the worst |b - b_ref| / (2^-53 absref_b) of the two barycentrics over the rays whose face equals the brute force's:
    b_ref the same quotient in extended precision, absref_b the sum of the absolute values of the six products of its
    numerator over |det|"""
    face = np.asarray(face, np.int64)
    same = np.flatnonzero((face == ref["face"]) & (face >= 0))
    if not len(same):
        return 0.0
    L = np.longdouble
    v, tr = np.asarray(v, np.float64), np.asarray(tr, np.int64)
    a, b, c = (v[tr[face[same], k]].astype(L) for k in range(3))
    oo, dd = np.asarray(o)[same].astype(L), np.asarray(d)[same].astype(L)
    e1, e2, s = b - a, c - a, oo - a
    p, q = np.cross(dd, e2), np.cross(s, e1)
    det = (e1 * p).sum(-1)
    uref, wref = (s * p).sum(-1) / det, (dd * q).sum(-1) / det

    def absdot3(x, y, z):                                           # sum_i |x_i| (|y_j z_k| + |y_k z_j|)
        x, y, z = np.abs(x), np.abs(y), np.abs(z)
        return (x[:, 0] * (y[:, 1] * z[:, 2] + y[:, 2] * z[:, 1]) + x[:, 1] * (y[:, 2] * z[:, 0] + y[:, 0] * z[:, 2]) +
                x[:, 2] * (y[:, 0] * z[:, 1] + y[:, 1] * z[:, 0]))
    au, aw = absdot3(s, dd, e2) / np.abs(det), absdot3(dd, s, e1) / np.abs(det)
    ru = np.abs(np.asarray(u)[same].astype(L) - uref) / (U * au)
    rw = np.abs(np.asarray(w)[same].astype(L) - wref) / (U * aw)
    return float(max(ru.max(), rw.max()))
