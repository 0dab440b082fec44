"""Restatement of the surface rasteriser (esr_nerf_amd/csrc/raster.hip, raster.py) by RAY CASTING, in numpy float64: no
projection, no edge function, no 1 / sum(b / z) -- nothing of the kernel's arithmetic.

For every pixel the ray of csrc/camera_ray.h is built in float64 from the binary32 camera (o = t, d = R (px, py, 1),
px = ((i + 0.5) - cx) / fx), intersected with every face (Moeller-Trumbore) and the nearest hit kept, ties to the smaller
face id.  d's camera-space z is 1, so the ray parameter t IS the camera depth the kernel stores.  The same two rules
bound what a face may do: a face with any vertex at camera depth <= z_near is dropped (and counted); a face the ray lies
in, or of zero area, has determinant 0 and is never hit.

Where another answer is legitimate the pixel is AMBIGUOUS and set aside with its acceptable answers:
  - some face with t > 0 has a barycentric with |b| < BAND (the centre is on an edge, to rounding), or
  - the two nearest hits lie within 2^-22 relative of each other (the binary32 key cannot tell them apart for sure).
Acceptable there: every face the ray may hit (all b >= -BAND) no farther than (1 + 2^-22) x the nearest SURE hit (all
b >= BAND), and "empty" when there is no sure hit.

Also here: the source masks / pixel counts in plain numpy, and the meshes and cameras the two test files share.
"""
import numpy as np

BAND = 1e-7
KEY_RES = 2.0 ** -22
DEPTH_BOUND = 2.0 ** -24 * (1 + 2.0 ** -20)          # one rounding of a float64 value to binary32


# ----------------------------------------------------------------------------------------------------------------------
# cameras and meshes


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """[3, 4] float32 camera-to-world pose in the kernels' convention (x right, y down, z forward)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.concatenate([np.stack([x, y, z], 1), eye[:, None]], 1).astype(np.float32)


class Cam:
    """a camera set in numpy: binary32 intrinsics and poses, as ``camera.Cameras`` holds them"""

    def __init__(self, poses, fx, fy, cx, cy, width, height):
        self.poses = np.asarray(poses, np.float32).reshape(-1, 3, 4)
        self.fx, self.fy, self.cx, self.cy = (float(np.float32(v)) for v in (fx, fy, cx, cy))
        self.width, self.height = int(width), int(height)

    @property
    def n_views(self):
        return self.poses.shape[0]

    def K(self):
        return np.array([[self.fx, 0, self.cx], [0, self.fy, self.cy], [0, 0, 1.0]])


def generic_cam(width=37, height=29, dist=3.2):
    """three views from outside the unit ball, fx != fy, the centre off the middle of the image"""
    poses = [look_at((dist, 0.3, 0.4), (0, 0, 0)), look_at((-0.9, dist * 0.8, -1.1), (0.05, 0, 0.1)),
             look_at((0.4, -1.0, dist * 0.9), (0, -0.05, 0), up=(0, 1, 0))]
    s = min(width, height)
    return Cam(poses, 1.25 * s, 1.1 * s, 0.5 * width + 1.3, 0.5 * height - 0.8, width, height)


def inside_cam(width=37, height=29):
    poses = [look_at((0.1, 0.05, -0.1), (1, 0.2, 0.1)), look_at((-0.1, 0.0, 0.12), (-0.3, -1, 0.2)),
             look_at((0.0, 0.1, 0.0), (0.1, 0.2, 1), up=(0, 1, 0))]
    return Cam(poses, 0.45 * width, 0.5 * width, 0.5 * width - 0.7, 0.5 * height + 1.1, width, height)


def lumpy_sphere(n_lon=12, n_stack=13, radius=1.0, lump=0.12, seed=0):
    """a closed sphere of 2 n_lon (n_stack - 1) faces (288) with a smooth radial bump, outward winding"""
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 2 * np.pi, 3)
    verts = [(0.0, 0.0, 1.0)]
    for s in range(1, n_stack):
        th = np.pi * s / n_stack
        for l in range(n_lon):
            lo = 2 * np.pi * (l + 0.5 * (s % 2)) / n_lon
            verts.append((np.sin(th) * np.cos(lo), np.sin(th) * np.sin(lo), np.cos(th)))
    verts.append((0.0, 0.0, -1.0))
    v = np.array(verts)
    r = radius * (1 + lump * (np.sin(3 * v[:, 0] + ph[0]) * np.cos(2 * v[:, 1] + ph[1]) + 0.5 * np.sin(4 * v[:, 2] + ph[2])))
    v = v * r[:, None] + np.array([0.013, -0.021, 0.008])
    ring = lambda s, l: 1 + (s - 1) * n_lon + l % n_lon
    t = []
    for l in range(n_lon):
        t.append((0, ring(1, l), ring(1, l + 1)))
        t.append((len(v) - 1, ring(n_stack - 1, l + 1), ring(n_stack - 1, l)))
    for s in range(1, n_stack - 1):
        for l in range(n_lon):
            a, b, c, d = ring(s, l), ring(s, l + 1), ring(s + 1, l), ring(s + 1, l + 1)
            t += [(a, c, b), (b, c, d)]
    return v.astype(np.float64), np.array(t, np.int64)


def blob_field(n=24):
    """an analytic float32 field on an n^3 lattice, positive inside two overlapping balls (for mesh.marching_cubes)"""
    g = np.stack(np.meshgrid(*[np.linspace(-1, 1, n)] * 3, indexing="ij"), -1)
    d0 = 0.62 - np.linalg.norm(g - np.array([0.12, 0.05, -0.1]), axis=-1)
    d1 = 0.4 - np.linalg.norm(g - np.array([-0.35, -0.3, 0.3]), axis=-1)
    return np.maximum(d0, d1).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# the ray cast


def pixel_rays(cam, view):
    """(o [3], d [P, 3]) of every pixel of a view in row order (pixel = j * width + i), float64 from the binary32 camera"""
    m = cam.poses[view].astype(np.float64)
    j, i = np.divmod(np.arange(cam.width * cam.height), cam.width)
    px = ((i + 0.5) - cam.cx) / cam.fx
    py = ((j + 0.5) - cam.cy) / cam.fy
    d = px[:, None] * m[None, :, 0] + py[:, None] * m[None, :, 1] + m[None, :, 2]
    return m[:, 3].copy(), d


def camera_depth(cam, view, points):
    """camera-space z of world points: the third component of M^-1 (p, 1), by solving, not by the kernel's matrix"""
    m = cam.poses[view].astype(np.float64)
    return np.linalg.solve(m[:, :3], (points - m[:, 3]).T)[2]


def _intersect(o, d, a, e1, e2):
    """Moeller-Trumbore of rays (o, d [P, 3]) with faces (a, e1, e2 [F, 3]) -> t, b0, b1, b2 [P, F] (NaN / inf where the
    determinant is 0: every comparison with them is false)"""
    p = np.cross(d[:, None, :], e2[None, :, :])
    det = (p * e1[None]).sum(-1)
    det = np.where(det == 0.0, np.nan, det)
    s = (o[None, :] - a)[None]
    u = (s * p).sum(-1) / det
    q = np.cross(s, e1[None])
    v = (d[:, None, :] * q).sum(-1) / det
    t = (e2[None] * q).sum(-1) / det
    return t, 1.0 - u - v, u, v


def _refine_t(o, d, v, tr, face):
    """t of ray k against face[k] in extended precision: a face thousands of image widths across loses five digits of t
    to cancellation in float64, more than the depth bound leaves beside binary32's half ulp"""
    L = np.longdouble
    a, b, c = (v[tr[face, k]].astype(L) for k in range(3))
    o, d = o.astype(L), d.astype(L)
    n = np.cross(b - a, c - a)
    return (((a - o[None]) * n).sum(-1) / (d * n).sum(-1)).astype(np.float64)


def cast_view(vertices, triangles, cam, view, z_near, face_chunk=None):
    """dict: face [P] int64 (-1: none), t [P] float64 (inf: none), ambiguous [P] bool, accept {pixel: (set of faces,
    empty_ok)} for the ambiguous pixels, n_dropped, hit [P, 3] the world point of the nearest hit"""
    v = np.asarray(vertices, np.float64)
    tr = np.asarray(triangles, np.int64).reshape(-1, 3)
    o, d = pixel_rays(cam, view)
    P, F = d.shape[0], tr.shape[0]
    face_chunk = face_chunk or max(1, (1 << 21) // P)          # [P, chunk] temporaries of a few tens of MB
    with np.errstate(all="ignore"):
        zc = camera_depth(cam, view, v) if len(v) else np.zeros(0)
        dropped = (zc[tr] <= z_near).any(1) if F else np.zeros(0, bool)
        live = np.flatnonzero(~dropped)
        t1, t2 = np.full(P, np.inf), np.full(P, np.inf)
        f1 = np.full(P, -1, np.int64)
        band = np.zeros(P, bool)
        for c0 in range(0, len(live), face_chunk):
            ids = live[c0:c0 + face_chunk]
            a = v[tr[ids, 0]]
            t, b0, b1, b2 = _intersect(o, d, a, v[tr[ids, 1]] - a, v[tr[ids, 2]] - a)
            bmin = np.minimum(np.minimum(b0, b1), b2)
            band |= ((t > 0) & (np.minimum(np.minimum(np.abs(b0), np.abs(b1)), np.abs(b2)) < BAND)).any(1)
            th = np.where((t > 0) & (bmin >= 0), t, np.inf)
            # the two nearest hits of this chunk, the nearest with the smallest id (ids ascend: argmin takes the first)
            k = np.argmin(th, 1)
            c1 = th[np.arange(P), k]
            th[np.arange(P), k] = np.inf
            c2 = th.min(1) if th.shape[1] > 1 else np.full(P, np.inf)
            better = c1 < t1                                   # (strict: an earlier chunk holds smaller ids)
            t2 = np.minimum(np.where(better, t1, c1), np.minimum(t2, c2))
            f1 = np.where(better, ids[k], f1)
            t1 = np.where(better, c1, t1)
        amb = band | (np.isfinite(t2) & (t2 - t1 <= KEY_RES * t1))
        got = np.flatnonzero(f1 >= 0)
        t1[got] = _refine_t(o, d[got], v, tr, f1[got])
        accept = {}
        rows = np.flatnonzero(amb)
        if len(rows):
            sure_t = np.full(len(rows), np.inf)
            maybe = []
            for c0 in range(0, len(live), face_chunk):
                ids = live[c0:c0 + face_chunk]
                a = v[tr[ids, 0]]
                t, b0, b1, b2 = _intersect(o, d[rows], a, v[tr[ids, 1]] - a, v[tr[ids, 2]] - a)
                bmin = np.minimum(np.minimum(b0, b1), b2)
                sure_t = np.minimum(sure_t, np.where((t > 0) & (bmin >= BAND), t, np.inf).min(1, initial=np.inf))
                r, c = np.nonzero((t > 0) & (bmin >= -BAND))
                maybe.append((r, ids[c], t[r, c]))
            for r, f, t in zip(*(np.concatenate(x) for x in zip(*maybe))) if maybe else ():
                if t <= sure_t[r] * (1 + KEY_RES):
                    accept.setdefault(int(rows[r]), (set(), not np.isfinite(sure_t[r])))[0].add(int(f))
            for r, p in enumerate(rows):
                accept.setdefault(int(p), (set(), not np.isfinite(sure_t[r])))
        hit = o[None, :] + np.where(np.isfinite(t1), t1, 0.0)[:, None] * d
    return dict(face=f1, t=t1, ambiguous=amb, accept=accept, n_dropped=int(dropped.sum()), hit=hit)


def cast(vertices, triangles, cam, z_near, views=None):
    return [cast_view(vertices, triangles, cam, v, z_near) for v in (range(cam.n_views) if views is None else views)]


def check_against(ref, face, depth, what=""):
    """the checks of one view: ``face`` / ``depth`` [P] of the code under test against ``ref`` (cast_view).  Returns the
    share of ambiguous pixels."""
    face, depth = np.asarray(face).reshape(-1), np.asarray(depth).reshape(-1)
    clear = ~ref["ambiguous"]
    bad = np.flatnonzero(clear & (face != ref["face"]))
    assert len(bad) == 0, (what, "face differs on unambiguous pixels", bad[:8], face[bad[:8]], ref["face"][bad[:8]])
    for p in np.flatnonzero(ref["ambiguous"]):
        faces, empty_ok = ref["accept"][int(p)]
        assert (face[p] in faces) or (face[p] == -1 and empty_ok), (what, "ambiguous pixel outside its set", int(p), int(face[p]),
                                                                    faces, empty_ok)
    assert np.array_equal(np.isposinf(depth), face == -1), (what, "depth is +inf exactly where there is no face")
    same = (face == ref["face"]) & (face >= 0)
    err = np.abs(depth[same].astype(np.float64) - ref["t"][same])
    worst = float((err / (DEPTH_BOUND * ref["t"][same])).max()) if same.any() else 0.0
    assert worst <= 1.0, (what, "depth is one rounding of the float64 value", worst)
    return float(ref["ambiguous"].mean()), worst


# ----------------------------------------------------------------------------------------------------------------------
# source masks


def source_masks(face, face_source, n_sources, groups):
    """face [v, H, W] -> (masks float32 [v, n_cond, H, W], pixels int64 [v, S])"""
    face = np.asarray(face)
    fs = np.asarray(face_source, np.int64)
    cond = np.full(n_sources, -1, np.int64)
    for c, g in enumerate(groups):
        cond[list(g)] = c
    src = np.where(face >= 0, fs[np.clip(face, 0, max(len(fs) - 1, 0))] if len(fs) else -1, -1)
    pc = np.where(src >= 0, cond[np.clip(src, 0, max(n_sources - 1, 0))] if n_sources else -1, -1)
    masks = np.stack([(pc == c).astype(np.float32) for c in range(len(groups))], 1) if len(groups) else \
        np.zeros((face.shape[0], 0) + face.shape[1:], np.float32)
    pixels = np.stack([np.bincount(s[s >= 0], minlength=n_sources)[:n_sources] for s in src.reshape(face.shape[0], -1)], 0) \
        if face.shape[0] else np.zeros((0, n_sources), np.int64)
    return masks, pixels.astype(np.int64).reshape(face.shape[0], n_sources)
