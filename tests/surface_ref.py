"""Restatement of the surface-component contract of esr_nerf_amd/csrc/meshcc.hip in numpy and plain Python, the meshes the
tests run it on, and mutants of the contract that the host tests must tell apart.

Contract: two SELECTED faces are connected iff they share a vertex id; an unselected face links nothing and is labelled
-1; a component is named by the smallest vertex id it contains and the components that own a selected face are numbered
0 .. K-1 in increasing order of that id.  Statistics per component over its faces: the face count, area = sum of
0.5 |(b - a) x (c - a)|, area_centroid = sum of area * ((a + b) + c) / 3, the bounding box of the face vertices, and
with an attribute [V, C]: area_attr = sum of area * (((x_a + x_b) + x_c) / 3) and peak = the largest attribute value at a
face vertex.  Every term is computed in float64 in the order written here (the kernel's order); the sums are
``math.fsum`` of the terms, i.e. exact.
"""
import math

import numpy as np

U = 2.0 ** -53            # unit roundoff of float64


# ----------------------------------------------------------------------------------------------------------------------
# connectivity


def _find(parent, v):
    r = v
    while parent[r] != r:
        r = parent[r]
    while parent[v] != r:
        parent[v], v = r, parent[v]
    return r


def components(triangles, n_vertices, face_mask=None, *, adjacency="vertex", order="min_vertex", unselected_link=False):
    """(face_label int32 [F], K).  The keyword arguments select MUTANTS of the contract (the defaults are the contract):
    ``adjacency="edge"``: faces are connected only across a shared edge; ``order="first_face"``: components numbered by
    their first face; ``unselected_link=True``: unselected faces join what they touch (and still get -1)."""
    tris = np.asarray(triangles, np.int64).reshape(-1, 3)
    n_f = len(tris)
    sel = np.ones(n_f, bool) if face_mask is None else np.asarray(face_mask).astype(bool).reshape(-1)
    link = np.ones(n_f, bool) if unselected_link else sel
    label = np.full(n_f, -1, np.int32)
    if adjacency == "vertex":
        parent = list(range(int(n_vertices)))
        for f in np.nonzero(link)[0]:
            a, b, c = (int(x) for x in tris[f])
            for x, y in ((a, b), (a, c)):
                rx, ry = _find(parent, x), _find(parent, y)
                if rx != ry:
                    parent[max(rx, ry)] = min(rx, ry)
        root = np.array([_find(parent, int(tris[f, 0])) if sel[f] else -1 for f in range(n_f)], np.int64)
    elif adjacency == "edge":
        parent = list(range(n_f))
        seen = {}
        for f in np.nonzero(link)[0]:
            a, b, c = (int(x) for x in tris[f])
            for e in ((a, b), (b, c), (a, c)):
                g = seen.setdefault((min(e), max(e)), int(f))
                rf, rg = _find(parent, int(f)), _find(parent, g)
                if rf != rg:
                    parent[max(rf, rg)] = min(rf, rg)
        # name of a face's component: the smallest vertex id over its faces
        froot = np.array([_find(parent, f) for f in range(n_f)], np.int64)
        name = {}
        for f in np.nonzero(link)[0]:
            name[froot[f]] = min(name.get(froot[f], 1 << 62), int(tris[f].min()))
        root = np.array([name[froot[f]] if sel[f] else -1 for f in range(n_f)], np.int64)
    else:
        raise ValueError(adjacency)
    owners = root[sel]
    if order == "min_vertex":
        names = np.unique(owners)
    elif order == "first_face":
        _, first = np.unique(owners, return_index=True)
        names = owners[np.sort(first)]
    else:
        raise ValueError(order)
    rank = {int(r): i for i, r in enumerate(names)}
    for f in np.nonzero(sel)[0]:
        label[f] = rank[int(root[f])]
    return label, len(names)


def components_scipy(triangles, n_vertices, face_mask=None):
    """the same labels from scipy.sparse.csgraph.connected_components on the vertex graph of the selected faces"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    tris = np.asarray(triangles, np.int64).reshape(-1, 3)
    sel = np.ones(len(tris), bool) if face_mask is None else np.asarray(face_mask).astype(bool).reshape(-1)
    t = tris[sel]
    i = np.concatenate([t[:, 0], t[:, 0], t[:, 1]])
    j = np.concatenate([t[:, 1], t[:, 2], t[:, 2]])
    g = coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n_vertices, n_vertices))
    _, vlab = connected_components(g, directed=False)
    # a scipy component's name: its smallest vertex id; only components with a selected face count
    smallest = np.full(vlab.max() + 1 if n_vertices else 0, n_vertices, np.int64)
    np.minimum.at(smallest, vlab, np.arange(n_vertices))
    label = np.full(len(tris), -1, np.int32)
    names = np.unique(smallest[vlab[t[:, 0]]]) if len(t) else np.zeros(0, np.int64)
    label[sel] = np.searchsorted(names, smallest[vlab[t[:, 0]]]).astype(np.int32)
    return label, len(names)


# ----------------------------------------------------------------------------------------------------------------------
# statistics


def face_terms(vertices, triangles, attr=None, *, half=True):
    """Per-face float64 terms in the kernel's operation order: dict(area [F], ac [F,3], lo [F,3], hi [F,3], aa [F,C],
    peak [F]).  ``half=False``: the MUTANT area without the factor 1/2."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    e1, e2 = b - a, c - a
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    area = (0.5 if half else 1.0) * np.sqrt((cx * cx + cy * cy) + cz * cz)
    out = dict(area=area, ac=area[:, None] * (((a + b) + c) / 3.0), lo=np.minimum(np.minimum(a, b), c),
               hi=np.maximum(np.maximum(a, b), c))
    if attr is not None:
        x = np.asarray(attr, np.float32).reshape(len(v), -1)
        x0, x1, x2 = x[t[:, 0]], x[t[:, 1]], x[t[:, 2]]
        out["aa"] = area[:, None] * (((x0.astype(np.float64) + x1.astype(np.float64)) + x2.astype(np.float64)) / 3.0)
        out["peak"] = np.maximum(np.maximum(x0, x1), x2).max(1) if len(t) else np.zeros(0, np.float32)
    return out


def _fsum_cols(x):
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    return np.array([math.fsum(x[:, k]) for k in range(x.shape[1])])


def stats(vertices, triangles, face_label, K, attr=None, *, half=True, weighted=True):
    """Per component: n_faces, area, area_centroid, centroid, bbox_min, bbox_max (and area_attr, mean_attr, peak) with
    exact sums, plus ``abs_*``: the sums of the absolute terms (the scale of the rounding bound).  ``weighted=False``: the
    MUTANT mean_attr that averages the face means without their areas."""
    lab = np.asarray(face_label).reshape(-1)
    T = face_terms(vertices, triangles, attr, half=half)
    C = T["aa"].shape[1] if attr is not None else 0
    out = dict(n_faces=np.zeros(K, np.int64), area=np.zeros(K), area_centroid=np.zeros((K, 3)), abs_area=np.zeros(K),
               abs_area_centroid=np.zeros((K, 3)), bbox_min=np.full((K, 3), np.inf), bbox_max=np.full((K, 3), -np.inf))
    if C:
        out.update(area_attr=np.zeros((K, C)), abs_area_attr=np.zeros((K, C)), peak=np.full(K, -np.inf, np.float32),
                   mean_attr=np.zeros((K, C)))
    order = np.argsort(lab, kind="stable")
    bounds = np.searchsorted(lab[order], np.arange(K + 1))
    for k in range(K):
        f = order[bounds[k]:bounds[k + 1]]
        out["n_faces"][k] = len(f)
        if not len(f):
            continue
        out["area"][k] = math.fsum(T["area"][f])
        out["abs_area"][k] = out["area"][k]
        out["area_centroid"][k] = _fsum_cols(T["ac"][f])
        out["abs_area_centroid"][k] = _fsum_cols(np.abs(T["ac"][f]))
        out["bbox_min"][k], out["bbox_max"][k] = T["lo"][f].min(0), T["hi"][f].max(0)
        if C:
            out["area_attr"][k] = _fsum_cols(T["aa"][f])
            out["abs_area_attr"][k] = _fsum_cols(np.abs(T["aa"][f]))
            out["peak"][k] = T["peak"][f].max()
            out["mean_attr"][k] = out["area_attr"][k] / out["area"][k] if weighted else \
                _fsum_cols(T["aa"][f] / T["area"][f][:, None]) / len(f)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["centroid"] = out["area_centroid"] / out["area"][:, None]
    return out


def sum_bound(n_faces, abs_sum):
    """|any-order float64 sum - exact sum| <= (n + 8) 2^-53 sum|terms|: the reorder bound of an n-term sum plus the
    roundings inside one term"""
    return (np.asarray(n_faces, np.float64).reshape(-1, *([1] * (np.ndim(abs_sum) - 1))) + 8.0) * U * np.asarray(abs_sum)


def sources(vertices, triangles, emission, k_val, min_area=0.0):
    """(face_source int32 [F], table): the emissive sources of esr_nerf_amd/sources.py restated"""
    em = np.asarray(emission, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    hot = em.max(1) > np.float32(k_val)
    sel = hot[t].all(1) if len(t) else np.zeros(0, bool)
    label, K = components(t, len(em), sel)
    st = stats(vertices, t, label, K, em)
    if min_area > 0.0 and K:
        keep = st["area"] >= min_area
        renum = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        label = np.where(label >= 0, renum[np.maximum(label, 0)], label).astype(np.int32)
        st = {k: v[keep] for k, v in st.items()}
    return label, st


# ----------------------------------------------------------------------------------------------------------------------
# meshes


def strip(n_tri, seed):
    """One strip of n_tri triangles (n_tri + 2 vertices) in one component, vertex ids permuted and faces shuffled: long
    parent chains and many compare-and-swap retries"""
    rng = np.random.default_rng(seed)
    i = np.arange(n_tri + 2)
    v = np.stack([(i // 2) * 0.75, (i % 2) * 1.25 + 0.1 * rng.random(len(i)), 0.5 * rng.random(len(i)) - 0.25], 1)
    t = np.stack([i[:-2], i[1:-1], i[2:]], 1)
    perm = rng.permutation(len(i))
    vv = np.empty_like(v)
    vv[perm] = v
    return vv, perm[t][rng.permutation(n_tri)].astype(np.int64)


def disjoint(n):
    """n single triangles that share nothing: n components, every lane of the statistics a different slot"""
    rng = np.random.default_rng(n)
    v = rng.random((3 * n, 3)) * 4.0 - 2.0
    t = np.arange(3 * n).reshape(n, 3)
    perm = rng.permutation(3 * n)
    vv = np.empty_like(v)
    vv[perm] = v
    return vv, perm[t].astype(np.int64)


def sheet_with_floaters(nx=37, ny=29, seed=4):
    """(vertices, triangles, face_mask): an nx x ny sheet of quads and five two-triangle floaters; the mask deselects one
    column of quads in the middle of the sheet (two halves that share no vertex) and the third floater"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    v = [np.stack([gx.ravel() * 0.3, gy.ravel() * 0.2, 0.05 * rng.standard_normal(gx.size)], 1)]
    vid = lambda i, j: i * (ny + 1) + j
    t, mask = [], []
    for i in range(nx):
        for j in range(ny):
            t += [(vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)), (vid(i, j), vid(i + 1, j + 1), vid(i, j + 1))]
            mask += [i != nx // 2] * 2
    n = gx.size
    for k in range(5):
        q = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0.5]], np.float64) * (0.2 + 0.1 * k) + [20.0 + 3 * k, k, 1.0]
        v.append(q)
        t += [(n, n + 1, n + 2), (n, n + 2, n + 3)]
        mask += [k != 2] * 2
        n += 4
    v, t, mask = np.concatenate(v), np.array(t, np.int64), np.array(mask, np.uint8)
    order = rng.permutation(len(t))           # floaters and sheet interleaved in the face list
    return v, t[order], mask[order]


def two_spheres_and_torus(R=48):
    """float32 field [R, R, R], > 0 inside two spheres and a torus that do not touch: three components"""
    x = np.linspace(-1.0, 1.0, R)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    s1 = 0.3 - np.sqrt((X + 0.55) ** 2 + (Y + 0.5) ** 2 + (Z + 0.45) ** 2)
    s2 = 0.2 - np.sqrt((X - 0.6) ** 2 + (Y - 0.6) ** 2 + (Z + 0.5) ** 2)
    tor = 0.12 - np.sqrt((np.sqrt(X ** 2 + Y ** 2) - 0.45) ** 2 + (Z - 0.45) ** 2)
    return np.maximum(np.maximum(s1, s2), tor).astype(np.float32)
