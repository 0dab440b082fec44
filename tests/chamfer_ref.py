"""numpy float64 restatement of the DTU Chamfer contract of esr_nerf_amd/csrc/chamfer.hip (the reference's
utils2.metric.DTU_CD with an explicit shuffle order).  Small inputs only: the downsample is the sequential keep loop over
a dict of cells and the nearest neighbour is brute force in chunks."""
import math

import numpy as np


def remove_unreferenced(vertices, triangles):
    used = np.zeros(len(vertices), dtype=bool)
    used[np.asarray(triangles).reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return np.asarray(vertices, np.float64)[used], remap[np.asarray(triangles, np.int64)]


def sample_points(vertices, triangles, thresh=0.2):
    """the referenced vertices, then per triangle with area2 > 0 the grid points (i, j) with a + b < 1, in numpy's
    operation order (np.linalg.norm, np.cross, np.mgrid)"""
    v, f = remove_unreferenced(vertices, triangles)
    tv = v[f]
    v1 = tv[:, 1] - tv[:, 0]
    v2 = tv[:, 2] - tv[:, 0]
    l1 = np.linalg.norm(v1, axis=-1)
    l2 = np.linalg.norm(v2, axis=-1)
    area2 = np.linalg.norm(np.cross(v1, v2), axis=-1)
    nz = area2 > 0
    l1, l2, area2, v1, v2, p0 = l1[nz], l2[nz], area2[nz], v1[nz], v2[nz], tv[nz, 0]
    thr = thresh * np.sqrt(l1 * l2 / area2)
    n1 = np.floor(l1 / thr)
    n2 = np.floor(l2 / thr)
    out = [v]
    for t in range(len(n1)):
        i, j = np.meshgrid(np.arange(n1[t] + 1), np.arange(n2[t] + 1), indexing="ij")
        a = (i.reshape(-1) + 0.5) / max(n1[t], 1e-7)
        b = (j.reshape(-1) + 0.5) / max(n2[t], 1e-7)
        k = a + b < 1
        a, b = a[k, None], b[k, None]
        out.append(v1[t] * a + v2[t] * b + p0[t])
    return np.concatenate(out, 0)


def d2(a, b):
    """((dx*dx + dy*dy) + dz*dz) of every pair, [len(a), len(b)]"""
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def downsample(points, thresh):
    """keep mask of the sequential loop: position k is kept unless a kept earlier position lies within thresh"""
    p = np.asarray(points, np.float64)
    h = thresh * (1.0 + 2.0 ** -20)
    o = p.min(0) if len(p) else np.zeros(3)
    cells = {}
    keep = np.zeros(len(p), dtype=bool)
    t2 = thresh * thresh
    c = np.floor((p - o) / h).astype(np.int64)
    for k in range(len(p)):
        cx, cy, cz = c[k]
        hit = False
        for x in (cx - 1, cx, cx + 1):
            for y in (cy - 1, cy, cy + 1):
                for z in (cz - 1, cz, cz + 1):
                    ids = cells.get((x, y, z))
                    if ids and (d2(p[k:k + 1], p[ids])[0] <= t2).any():
                        hit = True
                        break
                if hit:
                    break
            if hit:
                break
        if not hit:
            keep[k] = True
            cells.setdefault((cx, cy, cz), []).append(k)
    return keep


def nn(queries, targets, max_dist=20.0, chunk=2048):
    """sqrt(min squared distance) per query, inf where that is not < max_dist"""
    q = np.asarray(queries, np.float64).reshape(-1, 3)
    t = np.asarray(targets, np.float64).reshape(-1, 3)
    out = np.full(len(q), np.inf)
    if not len(t):
        return out
    for s in range(0, len(q), chunk):
        best = np.full(len(q[s:s + chunk]), np.inf)
        for u in range(0, len(t), chunk):
            best = np.minimum(best, d2(q[s:s + chunk], t[u:u + chunk]).min(1))
        d = np.sqrt(best)
        out[s:s + chunk] = np.where(d < max_dist, d, np.inf)
    return out


def filters(data_down, obs_mask, bb, res, patch=60):
    """(data_in, data_in_obs): bounds of the float32 BB, then the ObsMask lookup at np.around((p - BB0) / Res)"""
    BB = np.asarray(bb).astype(np.float32)
    inb = ((data_down >= BB[:1] - patch) & (data_down < BB[1:] + patch * 2)).sum(axis=-1) == 3
    data_in = data_down[inb]
    g = np.around((data_in - BB[:1]) / np.asarray(res, np.float64).reshape(1, -1)).astype(np.int64)
    ginb = ((g >= 0) & (g < np.expand_dims(obs_mask.shape, 0))).sum(axis=-1) == 3
    gi = g[ginb]
    in_obs = obs_mask[gi[:, 0], gi[:, 1], gi[:, 2]].astype(bool)
    return data_in, data_in[ginb][in_obs]


def above(stl, plane):
    P = np.asarray(plane, np.float64).reshape(4)
    return ((P[0] * stl[:, 0] + P[1] * stl[:, 1]) + P[2] * stl[:, 2]) + P[3] > 0


def _mean(d, max_dist):
    s = d[d < max_dist]
    return s.mean() if len(s) else math.nan


def dtu_cd(vertices, triangles, obs_mask, bb, res, stl, plane, order, max_dist=20.0, patch=60, thresh=0.2,
           detail=False):
    pts = sample_points(vertices, triangles, thresh)
    data = pts[np.asarray(order)]
    keep = downsample(data, thresh)
    data_in, data_in_obs = filters(data[keep], obs_mask, bb, res, patch)
    stl = np.asarray(stl, np.float64)
    d2s = nn(data_in_obs, stl, max_dist)
    s2d = nn(stl[above(stl, plane)], data_in, max_dist)
    a, b = _mean(d2s, max_dist), _mean(s2d, max_dist)
    out = (a, b, (a + b) / 2)
    return (out, dict(pts=pts, keep=keep, d2s=d2s, s2d=s2d)) if detail else out
