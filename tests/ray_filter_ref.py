"""Float64 restatement of the training-ray filter (esr_nerf_amd/csrc/rayfilter.hip) that CLASSIFIES each ray as firm keep,
firm drop or marginal, and the seeded scene / ray sets the filter's tests and tools share (numpy only; no GPU).

Why a classifier.  The filter's result is one bit per ray, decided by comparisons (sample inside the box? mask alpha >=
threshold? t_max <= t_min? how many steps?).  Two correct binary32 evaluations in different operation orders -- the
reference's torch ops, the torch restatement kept in the renderers, the kernel -- may put a value that lies ON a boundary on
different sides of it.  A ray whose every comparison is decided with room to spare must come out the same everywhere; only
the others may differ.  "Room to spare" is derived here from the binary32 rounding of the chains, with u = 2^-24 (half an
ulp of 1), NOT from what any implementation returns.

Point error eps_p (per sample, per axis, world units).  The inputs (o, d, box, stepdist) are binary32 values and enter the
float64 chain exactly, so the difference to a binary32 evaluation is rounding alone:
  t_min: (b - o) one rounding, / v one rounding -> 2u |t_min| (max / min / clamp add none);
  march point  start + dir * (stepdist * k):  d * t_min (3u |d t_min| with t_min's error), + o (u |start|), |d| = sqrt of
    three products and two sums (<= 3u), dir = d / |d| (4u), stepdist * k (u), dir * dist (6u dist in all), the final sum
    (u |p|): <= u (3 |d t_min| + |start| + 6 dist + |p|);
  fixed point  o + d * (t_min + (stepdist * k) / |d|):  t carries 2u |t_min| + 5u step / |d| + u |t|, the product with d one
    more u, the sum u |p|: <= u (9 |d| t + |p|).
With M = |o|_inf + |d|_inf * t (>= every magnitude above, t the sample's ray parameter) both are below 12 u M: "a few ulp of
the coordinate magnitude".  EPS_P_ULPS = 12.

Step count (march).  len = (t_max - t_min) |d| / stepdist carries 2u (|t_max| + |t_min|) |d| / stepdist from the two t's and
6u len from the difference, norm, product and quotient; a step index in [ceil(len - dl), ceil(len + dl)) may or may not exist.
Miss test (fixed).  t_max <= t_min is uncertain when |t_max - t_min| <= 4u (|t_max| + |t_min|), unless both unclamped ends
lie beyond far (or before near, near > 0) by more than 4u relative: then both clamp to the same bound and are equal exactly.

Mask alpha error eps_a (per sample).  alpha = 1 - exp(-softplus(x)) = sigmoid(x), x = density(p) + act_shift.
  density: the index chain ((p - lo) / (hi - lo)) * 2 - 1, ((n + 1) / 2) * (size - 1) has 6 roundings of values <= 2, so the
    continuous index is off by at most (6u * 2 + eps_p / (hi - lo)) * (size - 1) per axis; the trilinear field (zero padding
    included) is continuous and changes by at most G_a per unit index along axis a (G_a = the largest difference of adjacent
    nodes of the zero-padded grid along that axis); the corner weights are exact differences and the 8 taps add 2 roundings
    per weight product and one per fma: 16u D with D the largest |density|; x = density + shift adds u (D + |shift|).
  slope: sigmoid' = s (1 - s) <= min(s, 1/4) <= 1 and s grows with x, so over [x - dx, x + dx] the slope is at most
    min(sigmoid(x + dx), 1/4).
  tail: softplus = log1pf(expf(x)) to a few ulp of its value s, expf(-s) changes by at most exp(-s) (4u s + 2u) <= 4u, the
    final 1 - e is one rounding of a value <= 1: 8u in all.
  eps_a = min(sigmoid(x + dx), 1/4) * dx + 8u, dx = the density bound above.
A sample is a FIRM HIT when it certainly exists, lies inside every face by more than eps_p and alpha - thres > eps_a; it
FIRMLY FAILS when it certainly does not exist, or lies outside some face by more than eps_p, or thres - alpha > eps_a.
Ray: firm keep = some firm hit; firm drop = every sample firmly fails (a fixed-mode ray that certainly misses, or whose miss
test is uncertain but whose samples all fail anyway, is a firm drop); everything else is marginal.
"""

import numpy as np

U = 2.0 ** -24
EPS_P_ULPS = 12.0
KEEP, DROP, MARGINAL = 1, 0, -1
MARGINAL_CAP = 0.005          # largest marginal share of the large seeded set, per mode (a condition on the INPUTS)

SCENE = "tiny"                # synthetic.slab_scene: box (-1,-1,-.25)..(1,1,.25), world [64,64,16], prune mask
FAR = 3.2                     # the model's far: cuts the t-range of the rays that enter the box late (fixed mode only)


# ---------------------------------------------------------------------------------------------------------------------------
# scene and rays
# ---------------------------------------------------------------------------------------------------------------------------
def slab():
    from esr_nerf_amd.synthetic import slab_scene
    sc = slab_scene(SCENE, mask="prune")
    sc.far = FAR
    return sc


def scene_of(renderer):
    """The constants of a renderer (ours or the reference's, any device) the filter reads, as float64 / numpy"""
    f64 = lambda t: t.detach().cpu().double().numpy()
    dens = renderer.mask_cache.density.detach().cpu().numpy()[0, 0]
    return dict(xyz_min=f64(renderer.xyz_min), xyz_max=f64(renderer.xyz_max), mask_min=f64(renderer.mask_cache.xyz_min),
                mask_max=f64(renderer.mask_cache.xyz_max), density=dens.astype(np.float64), near=float(np.float32(renderer.near)),
                far=float(np.float32(renderer.far)),
                stepdist=float((renderer.stepsize * renderer.voxel_size.detach().cpu()).float()),
                act_shift=float(np.float32(renderer.mask_cache.act_shift)), thres=float(np.float32(renderer.mask_cache.mask_cache_thres)),
                n_samples=int(np.linalg.norm(np.array(renderer.sdf.grid.shape[2:]) + 1) / renderer.stepsize) + 1)


def look_at(eye, target=(0.0, 0.0, 0.0)):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, y, z, eye
    return P.astype(np.float32)


def camera_rays(pose, h, w, focal, jitter=None):
    """Pinhole rays of the datasets' convention: dirs = ((i - w/2) / f, -(j - h/2) / f, -1) rotated by the pose,
    un-normalised; one origin per pose.  float32 [h*w, 3] each."""
    j, i = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    if jitter is not None:
        i, j = i + jitter[0], j + jitter[1]
    dirs = np.stack([(i - w * 0.5) / focal, -(j - h * 0.5) / focal, -np.ones_like(i)], -1).astype(np.float32)
    rd = (dirs[..., None, :] * pose[:3, :3]).sum(-1).astype(np.float32).reshape(-1, 3)
    ro = np.broadcast_to(pose[:3, 3], rd.shape).astype(np.float32).copy()
    return ro, rd


POSES = [(2.3, -1.2, 1.4), (-1.9, 2.0, 0.9), (0.4, 2.6, -1.1), (-2.4, -0.7, 0.35)]


def large_set(seed=5, side=224):
    """~200 k camera rays: four poses around the box, side x side pixels each, sub-pixel offsets from the seed"""
    rng = np.random.default_rng(seed)
    ros, rds = [], []
    for eye in POSES:
        jit = rng.random((2, side, side)).astype(np.float32)
        ro, rd = camera_rays(look_at(eye, (0.1, -0.05, 0.0)), side, side, 0.9 * side, jit)
        ros.append(ro)
        rds.append(rd)
    return np.concatenate(ros), np.concatenate(rds)


# ---------------------------------------------------------------------------------------------------------------------------
# the classifier
# ---------------------------------------------------------------------------------------------------------------------------
def _trange(S, o, d, far):
    v = np.where(d == 0, float(np.float32(1e-6)), d)
    ta, tb = (S["xyz_max"] - o) / v, (S["xyz_min"] - o) / v
    lo, hi = np.minimum(ta, tb).max(-1), np.maximum(ta, tb).min(-1)
    return np.minimum(np.maximum(lo, S["near"]), far), np.minimum(np.maximum(hi, S["near"]), far), lo, hi


def _density(S, p):
    """Trilinear sample (align_corners, zero padding) of the mask density at world points p [m, 3], float64"""
    g = S["density"]
    dims = np.array(g.shape)
    idx = (p - S["mask_min"]) / (S["mask_max"] - S["mask_min"]) * (dims - 1)
    idx = np.clip(idx, -1.0, dims.astype(np.float64))          # beyond one cell outside everything is padding
    gp = np.pad(g, 1)
    i0 = np.floor(idx).astype(np.int64)
    i0 = np.minimum(i0, dims - 1)                              # idx == dims: weight 1 on the padding node either way
    f = idx - i0
    out = np.zeros(len(p))
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                w = (f[:, 0] if cx else 1 - f[:, 0]) * (f[:, 1] if cy else 1 - f[:, 1]) * (f[:, 2] if cz else 1 - f[:, 2])
                out += w * gp[i0[:, 0] + 1 + cx, i0[:, 1] + 1 + cy, i0[:, 2] + 1 + cz]
    return out


def _sigmoid(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def classify(S, rays_o, rays_d, fixed, chunk=8192):
    """-> dict(cls [n] in {KEEP, DROP, MARGINAL}, keep64 [n] bool, first64 [n] (first kept step of the float64 chain, -1),
    n64 [n] steps walked, last_in64 [n] last in-box step or -1)"""
    g = S["density"]
    dims = np.array(g.shape)
    gp = np.pad(g, 1)
    G = np.array([np.abs(np.diff(gp, axis=a)).max() for a in range(3)])
    D = float(np.abs(g).max())
    ext_m = S["mask_max"] - S["mask_min"]
    n = len(rays_o)
    cls = np.empty(n, np.int8)
    keep64, first64 = np.zeros(n, bool), np.full(n, -1, np.int64)
    n64, last_in = np.zeros(n, np.int64), np.full(n, -1, np.int64)
    for a in range(0, n, chunk):
        o, d = rays_o[a:a + chunk].astype(np.float64), rays_d[a:a + chunk].astype(np.float64)
        m = len(o)
        nrm = np.sqrt((d * d).sum(-1))
        with np.errstate(divide="ignore", invalid="ignore"):
            tmin, tmax, lo, hi = _trange(S, o, d, S["far"] if fixed else 1e9)
            if fixed:
                miss = tmax <= tmin
                miss_unsure = np.abs(tmax - tmin) <= 4 * U * (np.abs(tmax) + np.abs(tmin))
                # both ends clamped to the same bound with room to spare: t_max == t_min exactly, in any precision
                beyond = (np.minimum(lo, hi) > S["far"] * (1 + 4 * U)) | (np.maximum(lo, hi) < S["near"] * (1 - 4 * U))
                miss_unsure &= ~beyond
                n_lo = np.where(miss & ~miss_unsure, 0, S["n_samples"])
                n_hi = np.where(miss & ~miss_unsure, 0, S["n_samples"])
                n_own = np.where(miss, 0, S["n_samples"])
            else:
                ln = (tmax - tmin) * nrm / S["stepdist"]
                dl = 2 * U * (np.abs(tmax) + np.abs(tmin)) * nrm / S["stepdist"] + 6 * U * np.abs(ln)
                cl = lambda x: np.maximum(np.ceil(np.nan_to_num(x, nan=1.0)), 1.0).astype(np.int64)
                n_lo, n_hi, n_own = cl(ln - dl), cl(ln + dl), cl(ln)
                miss_unsure = np.zeros(m, bool)
        K = max(int(n_hi.max()) if m else 0, 1)          # (a column nobody owns keeps the reductions below defined)
        k = np.arange(K, dtype=np.float64)[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            if fixed:
                t = tmin[:, None] + (S["stepdist"] * k) / nrm[:, None]
                p = o[:, None, :] + d[:, None, :] * t[..., None]
            else:
                t = tmin[:, None] + (S["stepdist"] * k) / nrm[:, None]
                p = (o + d * tmin[:, None])[:, None, :] + (d / nrm[:, None])[:, None, :] * (S["stepdist"] * k)[..., None]
        eps_p = EPS_P_ULPS * U * (np.abs(o).max(-1)[:, None] + np.abs(d).max(-1)[:, None] * np.abs(t))
        mbox = np.minimum(p - S["xyz_min"], S["xyz_max"] - p).min(-1)          # > 0 inside
        sure_exists = k < n_lo[:, None]
        may_exist = k < n_hi[:, None]
        own = k < n_own[:, None]
        cand = may_exist & ~(mbox < -eps_p) & np.isfinite(mbox)                # not firmly outside
        ri, ki = np.nonzero(cand)
        alpha = np.zeros((m, K))
        eps_a = np.zeros((m, K))
        if len(ri):
            dens = _density(S, p[ri, ki])
            didx = (12 * U + eps_p[ri, ki, None] / ext_m) * (dims - 1)
            dx = (didx * G).sum(-1) + 16 * U * D + U * (D + abs(S["act_shift"]))
            x = dens + S["act_shift"]
            alpha[ri, ki] = _sigmoid(x)
            eps_a[ri, ki] = np.minimum(_sigmoid(x + dx), 0.25) * dx + 8 * U
        firm_hit = cand & sure_exists & (mbox > eps_p) & (alpha - S["thres"] > eps_a)
        firm_fail = ~cand | (S["thres"] - alpha > eps_a)
        hit64 = own & (mbox >= 0) & (alpha >= S["thres"])
        any_firm = firm_hit.any(-1)
        all_fail = firm_fail.all(-1)
        c = np.where(any_firm & ~miss_unsure, KEEP, np.where(all_fail, DROP, MARGINAL)).astype(np.int8)
        cls[a:a + m] = c
        keep64[a:a + m] = hit64.any(-1)
        first64[a:a + m] = np.where(hit64.any(-1), hit64.argmax(-1), -1)
        n64[a:a + m] = n_own
        inb = own & (mbox >= 0)
        last_in[a:a + m] = np.where(inb.any(-1), K - 1 - inb[:, ::-1].argmax(-1), -1)
    return dict(cls=cls, keep64=keep64, first64=first64, n64=n64, last_in64=last_in)


def agreement(cls, flags):
    """(number of firm rays whose flag disagrees with the classifier, marginal share)"""
    flags = np.asarray(flags).astype(bool)
    firm = cls != MARGINAL
    bad = int((flags[firm] != (cls[firm] == KEEP)).sum())
    return bad, float((~firm).mean()) if len(cls) else 0.0


def renderers(device, coarse_cls=None, fine_cls=None):
    """(VoxurfC, VoxurfF) on the shared scene -- this package's classes unless the reference's are handed in"""
    import torch
    from esr_nerf_amd.config import coarse_cfg, fine_cfg
    if coarse_cls is None:
        from esr_nerf_amd.voxurfc import VoxurfC as coarse_cls
        from esr_nerf_amd.voxurff import VoxurfF as fine_cls
    sc = slab()
    box = (sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max, sc.mask_alpha_init, sc.mask_density)
    torch.manual_seed(0)
    np.random.seed(0)
    coarse = coarse_cls(coarse_cfg(device, num_voxels=sc.num_voxels), *box, sc.s_val)
    fine = fine_cls(fine_cfg(device), *box, sc.s_val, sc.num_voxels)
    return coarse, fine
