"""float64 restatement of the stage hand-over kernels (esr_nerf_amd/csrc/gridsetup.hip), their binary32 emulation with its
mutants, and the inputs of tests/test_grid_setup_host.py and tests/test_gpu_grid_setup.py.

Resample (``esr_grid_resample``): the coordinates and the four lambdas per axis are formed in binary32 exactly as the kernel
forms them (``axis_coords``); the blend of the eight corners is taken in float64 (``resample_ref``) and comes with
``absref = sum |w| |v|``.  A binary32 blend commits one rounding for ``1 - l1`` and a product and a sum per level after it:
nine first-order roundings, each relative to at most absref, so ``|gpu - ref| <= 9 U absref`` (U = 2^-24) for every correct
implementation.  ``K_RESAMPLE`` is the next integer above the worst ratio measured on the MI355X and may not exceed 9.

Mask and bounds (``esr_nonempty_mask``, ``esr_density_bounds``): the continuous index per axis is formed in binary32 exactly
as ``esr_world_to_index`` forms it (``world_to_index``: numpy's float32 division is correctly rounded, as ``__fdiv_rn``); the
trilinear blend with zero padding and the activation are taken in float64 (``node_alpha``).  Each node carries a decision
BAND in alpha: ``4 U + (d alpha / d d) K_TRI U absref_d``.  The first term: ``1 - exp(-s)`` at s near the threshold cancels,
so the binary32 alpha is good to a few U absolute whatever its size (the rounding of exp(-s), of the subtraction, the ~3 ulp
of log1pf(expf(x)) scaled by s exp(-s) <= 0.37; the rounding of ``d + act_shift``, U |x| d alpha / d d, is far below one U at
the thresholds in use, where d alpha / d d is about alpha).  The second: the binary32 fetch commits two roundings for a
corner's weight product and one per fused accumulation, K_TRI = 10 first-order roundings relative to absref_d.  A node whose
float64 alpha lies within its band of the threshold may be decided either way; every other node must match.
"""
import math

import numpy as np

U = 2.0 ** -24
F32 = np.float32

# worst |gpu - ref| / (U absref) of esr_grid_resample on the MI355X per case of RESAMPLE_CASES (tests/test_gpu_grid_setup.py
# prints them; tools/stage_setup_time.py does not measure accuracy).  For orientation: CPU F.interpolate reaches 4.37 on the
# golden's shape, the plain binary32 emulation below 3.64.
MEASURED_RESAMPLE = {
    "2x1x3-5x1x7-c6": 1.478, "1x4x4-3x4x9-c1": 0.9048, "5x7x3-13x9x4-c1": 2.243, "33x17x9-20x40x9-c12": 2.754,
    "19x16x12-19x16x12-c1": 0.0, "19x16x12-19x16x12-c6": 0.0, "32x32x8-51x51x12-c6": 3.287,
    "40x40x10-129x128x64-c6": 4.311, "5x7x3-13x9x4-c5": 2.489,
}
# (the kernel's values equal the binary32 emulation's bit for bit on every case; the models' grids through
# DenseGrid.scale_volume_grid, (32,32,8) -> (50,50,12): sdf 3.499, off_color 3.526, emo_color 3.566)
K_RESAMPLE = 5                  # the next integer above the worst measured ratio, 4.311
K_RESAMPLE_CAP = 9              # the first-order rounding count: no measurement may lift K_RESAMPLE above it
K_TRI = 10

# (in, out, C): the table of the issue, then one channel count that takes the kernel's run-time-C path
RESAMPLE_CASES = [
    ((2, 1, 3), (5, 1, 7), 6),
    ((1, 4, 4), (3, 4, 9), 1),
    ((5, 7, 3), (13, 9, 4), 1),
    ((33, 17, 9), (20, 40, 9), 12),
    ((19, 16, 12), (19, 16, 12), 1),
    ((19, 16, 12), (19, 16, 12), 6),
    ((32, 32, 8), (51, 51, 12), 6),
    ((40, 40, 10), (129, 128, 64), 6),
    ((5, 7, 3), (13, 9, 4), 5),
]


def case_id(c):
    return "x".join(map(str, c[0])) + "-" + "x".join(map(str, c[1])) + f"-c{c[2]}"


def resample_input(case, seed=0):
    """[X,Y,Z,C] float32: a smooth field plus noise, both signs (so absref exceeds |ref| where values cancel)"""
    (X, Y, Z), _, C = case
    g = np.random.default_rng(1000 + seed + 7 * X + 11 * Y + 13 * Z + C)
    return (g.standard_normal((X, Y, Z, C)) * 2.0 + g.standard_normal((1, 1, 1, C))).astype(F32)


# ---- resample -----------------------------------------------------------------------------------------------------------------
def axis_coords(n_in, n_out, mutant=None, scale_of=None):
    """binary32 (i0, i1, l0, l1) per output index, as the kernel (and ATen's align_corners=True path) forms them;
    ``scale_of`` = (n_in, n_out) of ANOTHER axis to take the scale from (the swapped-axes mutant)"""
    dst = np.arange(n_out, dtype=F32)
    s_in, s_out = scale_of or (n_in, n_out)
    if mutant == "align_corners_false":
        scale = F32(s_in) / F32(s_out)
        src = np.maximum((scale * (dst + F32(0.5))).astype(F32) - F32(0.5), F32(0)).astype(F32)
    else:
        scale = F32(s_in - 1) / F32(s_out - 1) if s_out > 1 else F32(0)
        src = (scale * dst).astype(F32)
    if mutant == "round_half":
        i0 = np.floor(src + F32(0.5)).astype(np.int64)
    else:
        i0 = src.astype(np.int64)
    i0 = np.minimum(i0, n_in - 1)
    i1 = i0 + 1 if mutant == "i1_unclamped" else i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(F32)).astype(F32)
    l0 = (F32(1) - l1).astype(F32)
    return i0, i1, l0, l1


def _corners(vol, size, mutant=None):
    """the eight corner arrays [ox,oy,oz,C] (order x, y, z with z fastest) and the per-axis lambdas broadcast to them"""
    n_in = vol.shape[:3]
    ax = []
    for a in range(3):
        b = 2 - a if mutant == "swap_xz" else a          # the mutant scales x by z's sizes and z by x's
        ax.append(axis_coords(n_in[a], size[a], mutant, (n_in[b], size[b])))
    flat = vol.reshape(-1, vol.shape[3])
    if mutant == "i1_unclamped":         # flat memory: a read past the grid's end is a read of what lies behind it
        flat = np.concatenate([flat, np.full((n_in[1] * n_in[2] + n_in[2] + 2, vol.shape[3]), np.nan, vol.dtype)])
    sx, sy = n_in[1] * n_in[2], n_in[2]
    cs = []
    for k in range(8):
        ix = ax[0][(k >> 2) & 1][:, None, None]
        iy = ax[1][(k >> 1) & 1][None, :, None]
        iz = ax[2][k & 1][None, None, :]
        cs.append(flat[ix * sx + iy * sy + iz])
    lam = [(ax[0][2][:, None, None, None], ax[0][3][:, None, None, None]),
           (ax[1][2][None, :, None, None], ax[1][3][None, :, None, None]),
           (ax[2][2][None, None, :, None], ax[2][3][None, None, :, None])]
    return cs, lam


def resample_ref(vol, size):
    """(ref, absref) float64 [ox,oy,oz,C]: binary32 coordinates and lambdas, the blend in float64"""
    vol4 = vol if vol.ndim == 4 else vol[..., None]
    cs, lam = _corners(vol4.astype(np.float64), size)
    (x0, x1), (y0, y1), (z0, z1) = [(a.astype(np.float64), b.astype(np.float64)) for a, b in lam]

    def blend(v):
        return (x0 * (y0 * (z0 * v[0] + z1 * v[1]) + y1 * (z0 * v[2] + z1 * v[3])) +
                x1 * (y0 * (z0 * v[4] + z1 * v[5]) + y1 * (z0 * v[6] + z1 * v[7])))
    ref, absref = blend(cs), blend([np.abs(c) for c in cs])
    return (ref, absref) if vol.ndim == 4 else (ref[..., 0], absref[..., 0])


def resample_emul(vol, size, mutant=None):
    """the kernel's arithmetic in numpy binary32 (every product and sum rounded on its own)"""
    vol4 = vol if vol.ndim == 4 else vol[..., None]
    v, ((x0, x1), (y0, y1), (z0, z1)) = _corners(vol4.astype(F32), size, mutant)
    with np.errstate(invalid="ignore"):
        lo = y0 * (z0 * v[0] + z1 * v[1]) + y1 * (z0 * v[2] + z1 * v[3])
        hi = y0 * (z0 * v[4] + z1 * v[5]) + y1 * (z0 * v[6] + z1 * v[7])
        out = (x0 * lo + x1 * hi).astype(F32)
    return out if vol.ndim == 4 else out[..., 0]


def resample_ratio(got, ref, absref):
    """worst |got - ref| / (U absref); inf for a non-finite value or a difference where absref is 0"""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return math.inf
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(absref > 0, err / (U * absref), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


# ---- max pool -----------------------------------------------------------------------------------------------------------------
def maxpool_ref(vol, ks, pad_value=-np.inf):
    """max over the ks^3 window with a padding of ``pad_value`` (-inf: F.max_pool3d; 0 is the mutant)"""
    r = ks // 2
    p = np.pad(vol, r, constant_values=pad_value)
    out = np.full(vol.shape, -np.inf, vol.dtype)
    X, Y, Z = vol.shape
    for a in range(ks):
        for b in range(ks):
            for c in range(ks):
                out = np.maximum(out, p[a:a + X, b:b + Y, c:c + Z])
    return out


def maxpool_input(shape, seed=0):
    """random values with a block of -100, cells of +inf and -inf (all of it negative near the low corner: a zero
    padding would win there)"""
    g = np.random.default_rng(50 + seed + sum(shape))
    v = (g.standard_normal(shape) * 3 - 4).astype(F32)
    X, Y, Z = shape
    v[: max(1, X // 3), : max(1, Y // 3), : max(1, Z // 3)] = -100
    if v.size > 8:
        v[X // 2, Y // 2, Z // 2] = np.inf
        v[X - 1, Y - 1, 0] = -np.inf
        v[0, Y - 1, Z - 1] = -np.inf
    return v


MAXPOOL_SHAPES = [(19, 16, 12), (1, 1, 1), (2, 5, 1)]
MAXPOOL_KS = [1, 3, 5, 7]


# ---- mask cache lookup at lattice nodes ---------------------------------------------------------------------------------------
def world_to_index(p, lo, hi, n):
    """binary32 continuous index of the coordinates p (float32 vector) along one axis, as esr_world_to_index"""
    p, lo, hi = np.asarray(p, F32), F32(lo), F32(hi)
    u = ((p - lo) / (hi - lo)).astype(F32)
    nrm = (u * F32(2) - F32(1)).astype(F32)
    return (((nrm + F32(1)) / F32(2)).astype(F32) * F32(n - 1)).astype(F32)


def softplus64(x):
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def node_alpha(vol, box, act_shift, axes):
    """(alpha, band) float64 [X,Y,Z] at the nodes (axes[0][i], axes[1][j], axes[2][k]): binary32 index coordinates, the
    zero-padded trilinear blend of vol [mx,my,mz] and 1 - exp(-softplus(d + act_shift)) in float64; the decision band"""
    dims = vol.shape
    v64 = np.pad(vol.astype(np.float64), 1)                     # zero padding: index -1 and n
    per = []
    for a in range(3):
        idx = world_to_index(axes[a], box[a], box[3 + a], dims[a]).astype(np.float64)
        fl = np.floor(idx)
        i0 = fl.astype(np.int64)
        f = idx - fl
        w = [1.0 - f, f]
        ii = [np.clip(i0 + c, -1, dims[a]) + 1 for c in (0, 1)]      # (further out than one node: weightless zeros either way)
        far = [(i0 + c < -1) | (i0 + c > dims[a]) for c in (0, 1)]
        per.append((ii, w, far))
    d = np.zeros([len(a) for a in axes])
    absref = np.zeros_like(d)
    for cx in range(2):
        for cy in range(2):
            for cz in range(2):
                val = v64[per[0][0][cx][:, None, None], per[1][0][cy][None, :, None], per[2][0][cz][None, None, :]]
                out = per[0][2][cx][:, None, None] | per[1][2][cy][None, :, None] | per[2][2][cz][None, None, :]
                val = np.where(out, 0.0, val)
                w = per[0][1][cx][:, None, None] * per[1][1][cy][None, :, None] * per[2][1][cz][None, None, :]
                d += w * val
                absref += np.abs(w) * np.abs(val)
    x = d + float(F32(act_shift))
    sp = softplus64(x)
    alpha = -np.expm1(-sp)
    dalpha = np.exp(-sp) * np.where(x > 20.0, 1.0, 1.0 / (1.0 + np.exp(-np.minimum(x, 20.0))))
    band = 4 * U + dalpha * K_TRI * U * absref
    return alpha, band


def decide(alpha, band, thres, strict):
    """(decision, firm): the float64 decision (``>`` when strict, else ``>=``) and where the band does not reach thres"""
    t = float(F32(thres))
    dec = alpha > t if strict else alpha >= t
    return dec, np.abs(alpha - t) > band


def mask_emul(vol, box, act_shift, thres, axes, strict=False):
    """the mask kernel's decision from the float64 alpha rounded to binary32 (a stand-in for the device's alpha, exact
    enough for the host tests' mutants)"""
    alpha, _ = node_alpha(vol, box, act_shift, axes)
    a32 = alpha.astype(F32)
    return a32 > F32(thres) if strict else a32 >= F32(thres)


ALPHA_INIT, THRES = 1e-6, 1e-3                                  # alphamask.yaml's alpha_init, the stages' mask / bbox thresholds
ACT_SHIFT = math.log(1 / (1 - ALPHA_INIT) - 1)
MASK_BOX = (-1.0, -0.8, -0.6, 1.0, 0.9, 0.7)


def smooth_field(shape, seed, lo=-8.0, hi=12.0, knots=4):
    """a smooth random field spanning about lo .. hi: random knots resampled by the float64 restatement above"""
    g = np.random.default_rng(seed)
    k = g.uniform(lo, hi, (knots, knots, knots, 1)).astype(F32)
    ref, _ = resample_ref(k, shape)
    return np.ascontiguousarray(ref[..., 0].astype(F32))


def linspace32(lo, hi, n):
    import torch
    return torch.linspace(float(F32(lo)), float(F32(hi)), n).numpy()


def blob_field(shape, seed, peak=200.0, floor=-200.0, radius=0.12):
    """floor far from a random centre, peak at it (a Gaussian bump): a closed surface through the threshold whose area, and
    with it the expected number of band nodes, stays small however fine the lattice that looks it up (steep as well: the
    band is a few 1e-4 wide in density, a node's step across the surface tens of units)"""
    g = np.random.default_rng(seed)
    c = 0.5 + g.uniform(-0.08, 0.08, 3)
    ax = np.meshgrid(*[np.linspace(0, 1, n) for n in shape], indexing="ij")
    r2 = sum((a - c[i]) ** 2 for i, a in enumerate(ax))
    return np.ascontiguousarray((floor + (peak - floor) * np.exp(-r2 / (2 * radius ** 2))).astype(F32))


# name -> (SDF grid shape, SDF box, seed and kind of the pooled density (11,9,7)); the seeds are chosen so that at most 2
# nodes lie inside the band (tests/test_grid_setup_host.py::test_band_census holds them to it)
BOX_OUT, BOX_IN = (-1.3, -1.0, -0.8, 1.25, 1.1, 0.95), (-0.9, -0.7, -0.5, 0.85, 0.8, 0.65)
MASK_CASES = {
    "outside-19x16x12": ((19, 16, 12), BOX_OUT, 3, "smooth"),
    "inside-19x16x12": ((19, 16, 12), BOX_IN, 4, "smooth"),
    "outside-2x1x3": ((2, 1, 3), BOX_OUT, 5, "smooth"),
    "inside-2x1x3": ((2, 1, 3), BOX_IN, 16, "smooth"),
    "inside-129x128x64": ((129, 128, 64), BOX_IN, 7, "blob"),
}


def mask_input(name, axes=None):
    """dict(pooled [11,9,7], box, sdf_shape, sdf_box, axes): ``axes`` default to CPU torch.linspace (the GPU tests pass the
    device's arrays, which may differ from them in the last place)"""
    shape, sdf_box, seed, kind = MASK_CASES[name]
    pooled = smooth_field((11, 9, 7), 100 + seed) if kind == "smooth" else blob_field((11, 9, 7), 100 + seed)
    if axes is None:
        axes = [linspace32(sdf_box[a], sdf_box[3 + a], shape[a]) for a in range(3)]
    return dict(pooled=pooled, box=MASK_BOX, sdf_shape=shape, sdf_box=sdf_box, axes=axes)


# ---- bounds -------------------------------------------------------------------------------------------------------------------
BOUNDS_CASES = {
    "blob-19x16x12": ((19, 16, 12), "blob", 11),
    "one-cell": ((19, 16, 12), "one", 0),
    "corners": ((19, 16, 12), "corners", 0),
    "nothing": ((19, 16, 12), "nothing", 0),
    "blob-129x128x64": ((129, 128, 64), "blob", 12),
}


def bounds_density(name):
    shape, kind, seed = BOUNDS_CASES[name]
    X, Y, Z = shape
    if kind == "blob":
        g = np.random.default_rng(200 + seed)
        c = np.array([0.45, 0.55, 0.5]) + g.uniform(-0.1, 0.1, 3)
        ax = [np.linspace(0, 1, n) for n in shape]
        r2 = sum(((a - c[i]) / (0.22 + 0.05 * i)) ** 2 for i, a in
                 enumerate(np.meshgrid(*ax, indexing="ij")))
        bumps = smooth_field(shape, 300 + seed, -1.5, 1.5, 5)
        return np.ascontiguousarray((14.0 - 12.0 * r2 + bumps).clip(-10, 14).astype(F32))
    d = np.full(shape, -10.0, F32)
    if kind == "one":
        d[7, 3, 10] = 11.0
    elif kind == "corners":
        d[0, 0, 0] = 11.0
        d[X - 1, Y - 1, Z - 1] = 11.0
    return d


def bounds_axes32(box, shape):
    """CPU torch's lo * (1 - t) + hi * t (the GPU tests use the device's arrays instead)"""
    import torch
    out = []
    for a in range(3):
        t = torch.linspace(0, 1, shape[a])
        out.append((torch.tensor(box[a], dtype=torch.float32) * (1 - t) + torch.tensor(box[3 + a], dtype=torch.float32) * t).numpy())
    return out


def bounds_ref(density, box, act_shift, thres, axes):
    """dict(count_lo, count_hi, allowed): per output slot (min x, y, z, max x, y, z) the set of float32 values a correct
    kernel may return: the axis value at the extreme FIRM active index, or at a band node's index beyond it (a band node
    may move an extreme); count between the firm count and firm + band"""
    alpha, band = node_alpha(density, box, act_shift, axes)
    dec, firm = decide(alpha, band, thres, strict=True)
    sure = dec & firm
    maybe = ~firm
    allowed = []
    for hi_side in (False, True):
        for a in range(3):
            other = tuple(b for b in range(3) if b != a)
            s_idx = np.flatnonzero(sure.any(axis=other))
            m_idx = np.flatnonzero(maybe.any(axis=other))
            vals = set()
            if len(s_idx):
                e = s_idx[-1] if hi_side else s_idx[0]
                vals.add(float(axes[a][e]))
                vals |= {float(axes[a][i]) for i in m_idx if i == (e + 1 if hi_side else e - 1)}
            else:
                vals.add(-math.inf if hi_side else math.inf)
                vals |= {float(axes[a][i]) for i in m_idx}
            allowed.append(vals)
    return dict(count_lo=int(sure.sum()), count_hi=int(sure.sum() + (maybe).sum()), allowed=allowed, n_band=int(maybe.sum()))
