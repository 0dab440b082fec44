"""Restatement of the path-traced light on the surface (esr_nerf_amd/csrc/surfpath.hip, sources.path_light / lit_view(paths=)):
section X of include/esr_hip.h taken word by word in numpy and torch, with none of the kernel's machinery; never imported by
the product.

  philox       Philox4x32-10 on arrays of counters (the known answers are held in tests/test_surfpath_host.py)
  sphere       the direction sampler: Marsaglia's point on the sphere from the blocks 0 .. 7 of a counter, binary64, every
               operation on its own; sphere_from_words takes the words themselves (the fallback is reached by planting them)
  emulate      the kernel's ORDER of operations: decisions from raycast_ref.brute's binary64 triangle test (with its `ambiguous`
               flag), the binary32 flip, interpolation and back-face test (FLIP_BAND marks the values too near 0 to call), the
               BRDF from lts_ref64._disney in mode "32", surfenv_ref.env32 for the environment, section U's term in binary64,
               the lane's sums event by event in the kernel's order, and the balanced pairwise butterfly.  Its mutants stand
               for the mistakes a kernel of this kind can make
  reference    the same quantity in float64 at the emulation's decisions (directions, hits, slots, visibility), with `absref`
               from the error algebra lts_ref64.Q: the interpolated normal and material carry their binary32 roundings into one
               Disney chain per segment on the path's throughput, the J-term environment, section U's term (its Disney chain;
               the geometry is binary64), the binary64 sums' share and the final rounding
  check        the checks of tests/test_gpu_surfpath.py on one case: the emulation passes them (test_surfpath_host.py), every
               mutant fails one

Bound.  |out - ref64| <= K_FAMILY[family] 2^-24 absref per value, on every point none of whose paths holds an ambiguous
decision.  K is the smallest power of two at or above the worst ratio measured on the MI355X over every case of
tests/test_gpu_surfpath.py and for the emulation on the same cases.  The kernel's disney_eval is compiled with contraction,
expf / log1pf differ between the device's and the host's libraries by an ulp: the GPU is not bit-equal to the emulation where
either enters.  With D = 1, mode 1, a constant environment above the softplus threshold and no source nothing of that enters
and out is BIT-EQUAL to the emulation (`bitexact` cases).
"""
import math

import numpy as np
import torch

import lts_ref64 as lr
import raycast_ref as rr
import surfenv_ref as sv
import surflight_ref as sr

U24 = 2.0 ** -24
FLIP_BAND = sv.FLIP_BAND
MAX_PATHS, MAX_DEPTH = 4096, 8
TWO_PI = 2.0 * math.pi
INV2PI = sr.INV2PI
AMBIGUOUS_CAP = 0.01
COMPONENTS = ("env_dir", "env_indir", "src_indir")
# The worst |out - ref64| / (2^-24 absref) over every case of tests/test_gpu_surfpath.py (-s prints them) and, per family, the
# smallest power of two at or above it.  MI355X / the emulation on the same cases:
#   env          0.085 / 0.079   (the GPU's worst on "P=64", the emulation's in path_light's room)
#   src          0.118 / 0.060   (the GPU's worst in path_light's room, mode 0: its disney_eval is contracted, the emulation's is not)
#   irradiance   0.182 / 0.182   (on "tie": the final binary32 rounding of a bit-equal case)
# Far under 1 because absref counts every rounding of every Disney chain of a path, of the interpolated normal and material that
# enter it and of the 48-lobe sum at full magnitude, and the roundings of N paths average out in the mean.
K_FAMILY = {
    "env": 0.125,          # mode 0, the two environment components
    "src": 0.125,          # mode 0, the sources by way of another surface point
    "irradiance": 0.25,    # mode 1, all three components
}
MEASURED = {"env": (0.085, 0.079), "src": (0.118, 0.060), "irradiance": (0.182, 0.182)}   # MI355X, emulation

MUTANTS = ("no_flip", "flip_by_face_normal", "skip_not_updated", "wo_not_negated", "throughput_not_carried",
           "first_material_at_bounces", "nee_without_kp", "nee_at_first_vertex", "emission_on_source_hit", "miss0_in_indir",
           "divide_by_padded", "counter_without_b", "counter_without_point_base", "serial_sum", "mode1_weight_every_segment")

# the families a mutant is held against (a mutant of the sources' gather leaves the environment alone, and so on)
ALL = ("env", "src", "irradiance")
MUTANT_FAMILIES = {m: ALL for m in MUTANTS}
MUTANT_FAMILIES.update(nee_without_kp=("src", "irradiance"), nee_at_first_vertex=("src", "irradiance"),
                       emission_on_source_hit=("src", "irradiance"), miss0_in_indir=("env", "irradiance"), serial_sum=("irradiance",),
                       mode1_weight_every_segment=("irradiance",))

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def family(case, comp):
    return "irradiance" if case["mode"] == 1 else "env" if comp < 2 else "src"


def lanes(N):
    return min(64, sv.next_pow2(N))


# ----------------------------------------------------------------------------------------------------------------------
# random numbers


def philox(c0, c1, c2, c3, key):
    """uint32 [..., 4]: Philox4x32-10 of the counters (c0, c1, c2, c3), broadcast against each other, under key = (k0, k1)"""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(x).astype(np.uint64) & _MASK for x in (c0, c1, c2, c3)))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = c0 * np.uint64(M0), c2 * np.uint64(M1)
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def seed_key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def sphere_from_words(words):
    """(w f64 [..., 3], fallback bool [...]) from the words uint32 [..., B, 4] of the blocks 0 .. B - 1: per block the candidate
    pairs (w0, w1), (w2, w3); the first pair with s = a1 a1 + a2 a2 < 1 is taken"""
    a = 2.0 * (np.asarray(words, np.uint32).astype(np.float64) * 2.0 ** -32) - 1.0
    a = a.reshape(a.shape[:-2] + (-1, 2))                                   # the candidates in order
    w = np.zeros(a.shape[:-2] + (3,))
    w[..., 2] = 1.0
    taken = np.zeros(a.shape[:-2], bool)
    for j in range(a.shape[-2]):
        a1, a2 = a[..., j, 0], a[..., j, 1]
        s = a1 * a1 + a2 * a2
        ok = ~taken & (s < 1.0)
        q = np.sqrt(np.where(ok, 1.0 - s, 0.0))
        cand = np.stack([(2.0 * a1) * q, (2.0 * a2) * q, 1.0 - 2.0 * s], -1)
        w = np.where(ok[..., None], cand, w)
        taken |= ok
    return w, ~taken


def sphere(c0, c1, c2, key):
    """(w, fallback) of the counters (c0, c1, c2, .): the blocks 0 .. 7, each drawn only for the counters still without a pair"""
    c0, c1, c2 = (np.ascontiguousarray(a).reshape(-1) for a in np.broadcast_arrays(np.asarray(c0), np.asarray(c1), np.asarray(c2)))
    shape = np.broadcast(np.asarray(c0), np.asarray(c1), np.asarray(c2)).shape
    w = np.zeros((len(c0), 3))
    w[:, 2] = 1.0
    left = np.arange(len(c0))
    for blk in range(8):
        if not len(left):
            break
        got, fb = sphere_from_words(philox(c0[left], c1[left], c2[left], blk, key)[:, None, :])
        w[left[~fb]] = got[~fb]
        left = left[fb]
    fallback = np.zeros(len(c0), bool)
    fallback[left] = True
    return w.reshape(shape + (3,)), fallback.reshape(shape)


# ----------------------------------------------------------------------------------------------------------------------
# the pieces shared by the emulation and the reference


def _T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _dot32(a, b):
    s = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    assert s.dtype == np.float32
    return s


def disney32(base, rough, metal, n, wi, wo):
    """R f32 [m, 3] of m vertices, every operation a separately rounded binary32 one"""
    if not len(base):
        return np.zeros((0, 3), np.float32)
    f = lambda x: _T(np.asarray(x, np.float32))
    R = lr._disney(f(base)[:, None, :], f(rough)[:, None], f(metal)[:, None], f(n)[:, None, :], f(wi)[:, None, :], f(wo)[:, None, :], "32")
    return R.reshape(-1, 3).numpy()


def disney_q(base, rough, metal, n, wi, wo):
    """(R value f64 [m, 3], E [m, 3]) for the Q inputs base, n [m, 3], rough, metal [m] and the exact wi, wo f32 [m, 3]"""
    q = lambda x: lr.Q(_T(np.asarray(x, np.float32)).double())
    R = lr._disney(base[:, None, :], rough[:, None], metal[:, None], n[:, None, :], q(wi)[:, None, :], q(wo)[:, None, :], "q")
    return R.v.reshape(-1, 3).numpy(), R.E.reshape(-1, 3).numpy()


def face_unit_normals(v, tr):
    nv, ln = sr.face_normals(v, tr, np.arange(len(tr)))
    with np.errstate(all="ignore"):
        return (nv / ln[:, None]).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# the kernel's order of operations


def _lane_sum(ev, N, serial=False):
    """ev f64 [P, N, Ev, 3], the events of every path in the kernel's order -> [P, 3]: lane k adds the events of its paths k,
    k + Kd, ... one by one; the lanes are combined by the butterfly"""
    P, _, Ev, _ = ev.shape
    kd = lanes(N)
    trips = -(-N // kd)
    used = [e for e in range(Ev) if ev[:, :, e].any()]
    if serial:
        S = np.zeros((P, 3))
        for s in range(N):
            for e in used:
                S = S + ev[:, s, e]
        return S
    pad = np.zeros((P, trips * kd, Ev, 3))
    pad[:, :N] = ev
    pad = pad.reshape(P, trips, kd, Ev, 3)
    t = np.zeros((P, kd, 3))
    for i in range(trips):
        for e in used:
            t = t + pad[:, i, :, e]
    while t.shape[1] > 1:
        t = t[:, 0::2] + t[:, 1::2]
    return t[:, 0]


def emulate(case, mutant=None):
    """-> dict(out f32 [P, 3, 3], n_open i32 [P], trace i32 [P, N, D], end u8 [P, N], ambiguous bool [P, N], and what `reference`
    replays) of a case dict(v, tr, attrs = dict(normal, base, rough, metal: f32 per vertex), L (surflight_ref.lights) or None, sg
    or None, pts, nrm, face, mat (mode 0), mode, N, D, t_min, eps, seed, point_base, face_nrm; point_ids: the points' indices in
    the call they are taken from)"""
    v, tr, A, mode, N, D = case["v"], np.asarray(case["tr"], np.int64).reshape(-1, 3), case["attrs"], case["mode"], case["N"], case["D"]
    L, sg = case["L"], case["sg"]
    S, kp = (0, 1) if L is None else L["weight"].shape
    lgp = kp.bit_length() - 1
    J = 0 if sg is None else len(sg[0])
    pts, nrm = np.asarray(case["pts"], np.float64), np.asarray(case["nrm"], np.float32)
    P = len(pts)
    M = P * N
    f32 = np.float32
    pid, sid = np.repeat(np.arange(P), N), np.tile(np.arange(N), P)
    own = np.arange(P) if case.get("point_ids") is None else np.asarray(case["point_ids"], np.int64)   # (a subset of a larger call)
    ctr0 = own[pid] if mutant == "counter_without_point_base" else (case["point_base"] + own[pid])
    key = seed_key(case["seed"])
    x, n = pts[pid].copy(), nrm[pid].copy()
    if mode == 0:
        base, rough, metal, wo = (np.asarray(case["mat"][k], f32)[pid].copy() for k in ("base", "rough", "metal", "wo"))
    else:
        base, rough, metal, wo = np.zeros((M, 3), f32), np.zeros(M, f32), np.zeros(M, f32), np.zeros((M, 3), f32)
    base0, rough0, metal0 = base.copy(), rough.copy(), metal.copy()
    gn = np.asarray(case["face_nrm"], f32)[pid].copy()                      # (the geometric normal: a mutant flips by it)
    fun = face_unit_normals(v, tr) if len(tr) else np.zeros((0, 3), f32)
    face = np.full(M, -1, np.int64) if case["face"] is None else np.asarray(case["face"], np.int64)[pid].copy()
    T = np.ones((M, 3))
    active = np.ones(M, bool)
    trace, end, amb, open0 = np.full((M, D), -2, np.int32), np.zeros(M, np.uint8), np.zeros(M, bool), np.zeros(M, bool)
    ev_env, ev_src = np.zeros((M, 2, 1, 3)), np.zeros((M, (D + 1) * max(S, 1), 3))
    exact = bool(case.get("exact"))
    segs = []
    emit = {}
    if L is not None:
        for s in range(S):
            for k in range(kp):
                emit.setdefault(int(L["face"][s, k]), L["radiance"][s, k].astype(np.float64))

    def nee(idx, b, event0, first=False):
        """section U's term of one slot of every source at the vertices of the paths idx"""
        rec = []
        cb = 1 if mutant == "counter_without_b" else 2 * b + 1
        for s in range(S):
            word = philox(ctr0[idx], sid[idx], cb, s >> 2, key)[:, s & 3]
            k = (word >> np.uint32(32 - lgp)).astype(np.int64) if lgp else np.zeros(len(idx), np.int64)
            if case.get("force_slot") is not None:
                k[:] = case["force_slot"]                                  # (a test's hook: the mean over the slots)
            Aw, y, g, E, lf = L["weight"][s, k], L["point"][s, k], L["normal"][s, k], L["radiance"][s, k].astype(np.float64), L["face"][s, k]
            with np.errstate(all="ignore"):
                d = y - x[idx]
                r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                ws = d / np.sqrt(r2)[:, None]
                cos_l = -sr._dot(g, ws)
                cos_x = sr._dot(n[idx].astype(np.float64), ws)
                live = (Aw != 0.0) & (r2 > 0.0) & (cos_l > 0.0) & (cos_x > 0.0)
                G = (cos_l * Aw) / np.fmax(r2, Aw)
            li = np.flatnonzero(live)
            if not len(li):
                continue
            br = rr.brute(v, tr, x[idx][li], d[li], case["eps"], 1.0 - case["eps"], lf[li].astype(np.int64))
            if not exact:
                amb[idx[li]] |= br["ambiguous"]
            vi = li[~br["hit"]]
            if not len(vi):
                continue
            q = idx[vi]
            wl = ws[vi].astype(f32)
            R = disney32(base[q], rough[q], metal[q], n[q], wl, wo[q]).astype(np.float64)
            term = ((R * INV2PI) * G[vi][:, None]) * E[vi]
            if first and mode == 1:
                term = (cos_x[vi] * G[vi])[:, None] * E[vi]                # (the mutant's gather at a point of irradiance: section U's mode 1)
            ev_src[q, event0 + s] = T[q] * ((1.0 if mutant == "nee_without_kp" else float(kp)) * term)
            rec.append(dict(q=q, wl=wl, c=(INV2PI * G[vi])[:, None] * E[vi], event=event0 + s))
        return rec

    if mutant == "nee_at_first_vertex" and S:
        nee(np.arange(M), 0, 0, first=True)
    for b in range(D):
        idx = np.flatnonzero(active)
        if not len(idx):
            break
        w, _ = sphere(ctr0[idx], sid[idx], 0 if mutant == "counter_without_b" else 2 * b, key)
        wi = w.astype(f32)
        s = _dot32(wi, gn[idx] if mutant == "flip_by_face_normal" else n[idx])
        neg = (s < 0) & (mutant != "no_flip")
        w, wi = np.where(neg[:, None], -w, w), np.where(neg[:, None], -wi, wi)
        if not exact:
            amb[idx] |= np.abs(s) <= f32(FLIP_BAND)
        cos_x = sr._dot(n[idx].astype(np.float64), wi.astype(np.float64))
        irr = mode == 1 and (b == 0 or mutant == "mode1_weight_every_segment")
        if irr:
            Wt = np.repeat((cos_x * TWO_PI)[:, None], 3, 1)
        else:
            Wt = disney32(base[idx], rough[idx], metal[idx], n[idx], wi, wo[idx]).astype(np.float64)
        if mutant == "throughput_not_carried":
            T[idx] = 1.0
        with np.errstate(all="ignore"):
            T[idx] = T[idx] * Wt
        br = rr.brute(v, tr, x[idx], w, case["t_min"], np.inf, face[idx])
        if not exact:
            amb[idx] |= br["ambiguous"]
        hit = br["hit"]
        trace[idx, b] = np.where(hit, br["face"], -1)
        mi = idx[~hit]
        comp = 0 if b == 0 and mutant != "miss0_in_indir" else 1
        Lenv = None
        if J and len(mi):
            Lenv = sv.env32(sg, wi[~hit]).astype(np.float64)
            with np.errstate(all="ignore"):
                ev_env[mi, comp, 0] = T[mi] * Lenv
        if b == 0:
            open0[mi] = True
        end[mi], active[mi] = 1, False
        seg = dict(idx=idx, wi=wi, irr=irr, cos_x=cos_x, miss=mi, miss_wi=wi[~hit], comp=comp, nee=[])
        hi = idx[hit]
        if len(hi):
            f, u, vv = br["face"][hit], br["u"][hit], br["v"][hit]
            wts = np.stack([(1.0 - u) - vv, u, vv], 1)
            ids = tr[f]
            xn = (wts[:, 0:1] * v[ids[:, 0]] + wts[:, 1:2] * v[ids[:, 1]]) + wts[:, 2:3] * v[ids[:, 2]]
            w32 = wts.astype(f32)
            at = lambda a: (w32[:, 0:1] * a[ids[:, 0]] + w32[:, 1:2] * a[ids[:, 1]]) + w32[:, 2:3] * a[ids[:, 2]]
            nn = at(np.asarray(A["normal"], f32))
            with np.errstate(all="ignore"):
                ln = np.sqrt((nn[:, 0] * nn[:, 0] + nn[:, 1] * nn[:, 1]) + nn[:, 2] * nn[:, 2])
                ok = (ln > 0) & np.isfinite(ln)
                n_new = nn / ln[:, None]
                wo_new = wi[hit] if mutant == "wo_not_negated" else -wi[hit]
                dt = _dot32(n_new, wo_new)
                alive = ok & (dt > 0)
            assert n_new.dtype == f32
            if not exact:
                amb[hi] |= ok & (np.abs(dt) <= f32(FLIP_BAND))
            dead, go = hi[~alive], hi[alive]
            end[dead], active[dead] = 2, False
            x[go], n[go], wo[go] = xn[alive], n_new[alive], wo_new[alive]
            g = fun[f[alive]]
            gn[go] = np.where((_dot32(g, wo_new[alive]) < 0)[:, None], -g, g)
            if mutant != "skip_not_updated":
                face[go] = f[alive]
            if mutant != "first_material_at_bounces":
                base[go], rough[go], metal[go] = at(np.asarray(A["base"], f32))[alive], at(np.asarray(A["rough"], f32)[:, None])[alive, 0], \
                    at(np.asarray(A["metal"], f32)[:, None])[alive, 0]
            seg.update(go=go, ids=ids[alive], wts=wts[alive], T=T[go].copy(),
                       vertex=dict(x=x[go].copy(), n=n[go].copy(), base=base[go].copy(), rough=rough[go].copy(), metal=metal[go].copy(), wo=wo[go].copy()))
            if S and len(go):
                seg["nee"] = nee(go, b, (b + 1) * S)
            if mutant == "emission_on_source_hit":
                for j, q in enumerate(go):
                    if int(f[alive][j]) in emit:
                        ev_src[q, (b + 1) * max(S, 1)] += T[q] * emit[int(f[alive][j])]
        segs.append(seg)
    sh = lambda a: a.reshape((P, N) + a.shape[1:])
    serial = mutant == "serial_sum"
    with np.errstate(all="ignore"):
        sums = np.stack([_lane_sum(sh(ev_env[:, 0]), N, serial), _lane_sum(sh(ev_env[:, 1]), N, serial),
                         _lane_sum(sh(ev_src), N, serial)], 1)
        kd = lanes(N)
        out = (sums / float(kd * -(-N // kd) if mutant == "divide_by_padded" else N)).astype(f32)
    if not J:
        out[:, :2] = 0.0                                                   # (nothing is added without an environment: +0)
    return dict(out=out, n_open=sh(open0).sum(1).astype(np.int32), trace=sh(trace), end=sh(end), ambiguous=sh(amb), segs=segs,
                terms=sh(ev_env[:, :, 0]), base0=base0, rough0=rough0, metal0=metal0)


def reference(case, emu):
    """(value f64 [P, 3, 3], absref [P, 3, 3]) at the emulation's decisions"""
    A, mode, N, L, sg = case["attrs"], case["mode"], case["N"], case["L"], case["sg"]
    P = len(case["pts"])
    M = P * N
    kp = 1 if L is None else L["weight"].shape[1]
    if not M:
        return np.zeros((P, 3, 3)), np.zeros((P, 3, 3))
    Q = lr.Q
    pid = np.repeat(np.arange(P), N)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    # the vertex's normal and material: value and error (the first vertex is given: exact)
    st = {k: [_T(np.asarray(a, np.float64)), z(*a.shape)] for k, a in
          (("n", np.asarray(case["nrm"], np.float32)[pid]), ("base", emu["base0"]), ("rough", emu["rough0"]), ("metal", emu["metal0"]))}
    wo = np.zeros((M, 3), np.float32) if mode == 1 else np.asarray(case["mat"]["wo"], np.float32)[pid].copy()
    Tv, TE = np.ones((M, 3)), np.zeros((M, 3))
    val, err, mag = np.zeros((M, 3, 3)), np.zeros((M, 3, 3)), np.zeros((M, 3, 3))
    get = lambda k, q: Q(st[k][0][q], st[k][1][q])
    for seg in emu["segs"]:
        idx, wi = seg["idx"], seg["wi"]
        if seg["irr"]:
            Rv, RE = np.repeat((seg["cos_x"] * TWO_PI)[:, None], 3, 1), np.zeros((len(idx), 3))
        else:
            Rv, RE = disney_q(get("base", idx), get("rough", idx), get("metal", idx), get("n", idx), wi, wo[idx])
        TE[idx] = TE[idx] * np.abs(Rv) + np.abs(Tv[idx]) * RE
        Tv[idx] = Tv[idx] * Rv
        mi = seg["miss"]
        if sg is not None and len(mi):
            e_v, e_E = sv.env_ref(sg, seg["miss_wi"])
            c = seg["comp"]
            val[mi, c] = Tv[mi] * e_v
            err[mi, c] = TE[mi] * np.abs(e_v) + np.abs(Tv[mi]) * e_E
            mag[mi, c] = np.abs(val[mi, c])
        if "go" not in seg or not len(seg["go"]):
            continue
        go, ids, wts = seg["go"], seg["ids"], seg["wts"]
        wq = Q(_T(wts), _T(np.where(wts.astype(np.float32).astype(np.float64) == wts, 0.0, np.abs(wts))))
        at = lambda a: (wq[:, 0:1] * Q(_T(a[ids[:, 0]]).double()) + wq[:, 1:2] * Q(_T(a[ids[:, 1]]).double())) + wq[:, 2:3] * Q(_T(a[ids[:, 2]]).double())
        nn = at(np.asarray(A["normal"], np.float32))
        ll = nn * nn
        nq = nn / lr.xsqrt((ll[:, 0] + ll[:, 1]) + ll[:, 2])[:, None]
        new = dict(n=nq, base=at(np.asarray(A["base"], np.float32)), rough=at(np.asarray(A["rough"], np.float32)[:, None])[:, 0],
                   metal=at(np.asarray(A["metal"], np.float32)[:, None])[:, 0])
        for k, qv in new.items():
            st[k][0][go], st[k][1][go] = qv.v, qv.E
        loc = np.full(M, -1)
        loc[idx] = np.arange(len(idx))
        wo[go] = -wi[loc[go]]
        for rec in seg["nee"]:
            q, c = rec["q"], rec["c"]
            Rv, RE = disney_q(get("base", q), get("rough", q), get("metal", q), get("n", q), rec["wl"], wo[q])
            term = float(kp) * Rv * c
            val[q, 2] += Tv[q] * term
            err[q, 2] += float(kp) * np.abs(c) * (TE[q] * np.abs(Rv) + np.abs(Tv[q]) * RE)
            mag[q, 2] += np.abs(Tv[q] * term)
    sh = lambda a: a.reshape(P, N, 3, 3)
    value = sh(val).sum(1) / N
    # the binary64 chains (under 64 roundings of 2^-53 on magnitudes: 64 2^-29 in units of 2^-24) and the final rounding
    absref = (sh(err).sum(1) + 64 * 2.0 ** -29 * sh(mag).sum(1)) / N + np.abs(value)
    return value, absref


def check(case, out, n_open=None, trace=None, end=None, emu=None, what="", families=None):
    """The GPU's checks of one case -> (worst ratio per family, ambiguous paths); raises AssertionError.  `families`: the bound
    is asserted for these only (the mutants are held against one family at a time)"""
    emu = emu or emulate(case)
    out = np.asarray(out)
    assert out.dtype == np.float32 and out.shape == emu["out"].shape, (what, out.dtype, out.shape)
    amb = emu["ambiguous"]
    clear = ~amb.any(1)
    assert amb.sum() <= AMBIGUOUS_CAP * max(amb.size, 1) or case.get("constructed"), (what, "ambiguous paths over the cap", int(amb.sum()), amb.size)
    if trace is not None:
        trace = np.asarray(trace)
        assert trace.dtype == np.int32 and trace.shape == emu["trace"].shape, (what, trace.dtype, trace.shape)
        assert np.array_equal(trace[~amb], emu["trace"][~amb]), (what, "trace differs on unambiguous paths", int((trace != emu["trace"]).any(-1)[~amb].sum()))
    if end is not None:
        end = np.asarray(end)
        assert end.dtype == np.uint8 and end.shape == emu["end"].shape, (what, end.dtype, end.shape)
        assert np.array_equal(end[~amb], emu["end"][~amb]), (what, "end differs on unambiguous paths")
    if n_open is not None:
        n_open = np.asarray(n_open)
        assert n_open.dtype == np.int32 and n_open.shape == emu["n_open"].shape, (what, n_open.dtype, n_open.shape)
        mine = (emu["trace"][:, :, 0] == -1) if emu["trace"].shape[2] else np.zeros(amb.shape, bool)
        lo = (mine & ~amb).sum(1)
        hi = lo + amb.sum(1)
        assert ((lo <= n_open) & (n_open <= hi)).all(), (what, "n_open", n_open[:4], lo[:4], hi[:4])
    if case["sg"] is None:
        assert (out[:, :2].view(np.uint32) == 0).all(), (what, "the environment components are +0 without an environment")
    if case["L"] is None:
        assert (out[:, 2].view(np.uint32) == 0).all(), (what, "src_indir is +0 without a source")
    if case.get("bitexact"):
        bad = np.argwhere((out.view(np.uint32) != emu["out"].view(np.uint32)).any((1, 2)) & clear)
        assert len(bad) == 0, (what, "not bit-equal to the emulation", out[bad[:2, 0]].tolist(), emu["out"][bad[:2, 0]].tolist())
    value, absref = reference(case, emu)
    err = np.abs(out.astype(np.float64) - value)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(absref > 0, err / np.maximum(U24 * absref, 1e-300), np.where(err > 0, np.inf, 0.0))[clear]
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    worst = {}
    for comp in range(3):
        fam = family(case, comp)
        worst[fam] = max(worst.get(fam, 0.0), float(ratio[:, comp].max()) if ratio.size else 0.0)
    for fam, w in worst.items():
        assert (families is not None and fam not in families) or w <= K_FAMILY[fam], (what, "the bound does not hold", fam, w, K_FAMILY[fam])
    return worst, int(amb.sum())


# ----------------------------------------------------------------------------------------------------------------------
# scenes, attributes, lights, points and cases


def vertex_attrs(v, tr, seed=0):
    """per vertex: a normal turned into the scene's middle and tilted a little, and a random material"""
    rng = np.random.default_rng(seed + 50)
    V = len(v)
    vn = np.zeros((V, 3))
    if len(tr):
        nv, ln = sr.face_normals(v, tr, np.arange(len(tr)))
        mid = v.mean(0)
        for f in range(len(tr)):
            g = nv[f] / ln[f]
            vn[tr[f]] = -g if ((mid - v[tr[f, 0]]) * g).sum() < 0 else g       # (the room's quads own their vertices)
    else:
        vn[:, 2] = 1.0
    return dict(normal=sr.unit32(vn + 0.05 * rng.uniform(-1, 1, (V, 3))), base=rng.uniform(0.1, 0.9, (V, 3)).astype(np.float32),
                rough=rng.uniform(0.2, 0.9, V).astype(np.float32), metal=rng.uniform(0, 1, V).astype(np.float32))


def room_scene(window=False):
    """(v, tr, face_source, S): raycast_ref.room(), every quad split 2 x 2; with `window` the ceiling patch's faces are taken out,
    so that the sky is seen from inside, and the wall patch is the one source"""
    v, tr, fs, S = sr.refined_room(2)
    if window:
        keep = fs != 0
        tr, fs, S = tr[keep], np.where(fs[keep] == 1, 0, -1).astype(np.int32), 1
    return v, tr, fs, S


def one_face_scene():
    v, tr = sv.one_face()
    return v, tr, np.full(1, -1, np.int32), 0


def no_face_scene():
    v, tr = sv.no_face()
    return v, tr, np.zeros(0, np.int32), 0


_scenes = {}


def scene(name):
    if name not in _scenes:
        sc = {"room": room_scene, "window": lambda: room_scene(True), 1: one_face_scene, 0: no_face_scene}[name]()
        attrs = vertex_attrs(sc[0], sc[1], 2)
        if name == 1:
            attrs["normal"] = sr.unit32(np.array([[0.05, 0.0, -1.0], [0.0, 0.1, -1.0], [-0.1, 0.05, -1.0]]))
        _scenes[name] = (sc, attrs)
    return _scenes[name]


def scene_lights(name, S, kp, seed=0):
    """the lights of a scene with S sources of kp slots: the scene's own sources first, then copies of them with other radiances;
    under the one face a single planted light"""
    if S == 0:
        return None
    (v, tr, fs, S0), _ = scene(name)
    if S0 == 0:
        rng = np.random.default_rng(seed)
        L = dict(point=np.tile([0.7, 0.6, 0.1], (S, kp, 1)) + 0.2 * rng.uniform(-1, 1, (S, kp, 3)), normal=np.tile([0.0, 0.0, 1.0], (S, kp, 1)),
                 weight=np.full((S, kp), 0.02), radiance=rng.uniform(0.5, 4.0, (S, kp, 3)).astype(np.float32), face=np.full((S, kp), -1, np.int32))
        return L
    L0 = sr.lights(v, tr, fs, S0, kp, sr.vertex_emission(v, tr, fs, seed))
    pick = [s % S0 for s in range(S)]
    L = {k: L0[k][pick].copy() for k in ("point", "normal", "weight", "radiance", "face")}
    for s in range(S0, S):
        L["radiance"][s] = (L["radiance"][s] * np.float32(0.3 + 0.2 * s)).astype(np.float32)
    return L


def points(name, P, seed):
    pts, nrm = sv.room_points(P, seed)
    if name in (0, 1):
        pts[:, 2] = np.abs(pts[:, 2] - 1.0) * 0.3                          # under the face, most of them
        pts[:, :2] = 0.3 + pts[:, :2] * 0.25
        nrm = sr.unit32(nrm + np.array([0.0, 0.0, 1.2]))
    elif name == "window":
        pts[:, 2] = np.minimum(pts[:, 2], 2.3)                             # all inside: the sky through the window
    return pts, nrm


def make_case(name="room", P=5, N=16, D=2, S=2, kp=16, J=48, mode=0, seed=None, point_base=0, t_min=1e-3, eps=1e-3, pts=None, nrm=None,
              sg=None, seed_is=None, **flags):
    (v, tr, fs, _), attrs = scene(name)
    seed = 1000 * P + 10 * N + D + 7 * S + kp + J + 3 * mode if seed is None else seed
    if pts is None:
        pts, nrm = points(name, P, seed)
    pts, nrm = np.asarray(pts, np.float64).reshape(-1, 3), np.asarray(nrm, np.float32).reshape(-1, 3)
    case = dict(v=v, tr=tr, attrs=attrs, L=scene_lights(name, S, kp, seed), sg=sg if sg is not None else (sv.sg_random(J, seed) if J else None),
                pts=pts, nrm=nrm, face=None, mode=mode, N=N, D=D, t_min=t_min, eps=eps,
                seed=0x9E3779B97F4A7C15 ^ seed if seed_is is None else seed_is, point_base=point_base,
                face_nrm=nrm.copy(), scene=name)
    if mode == 0:
        case["mat"] = sr.materials(len(pts), pts, seed + 1)
    case.update(flags)
    return case


def on_mesh_case(mode, name="window"):
    """points ON the mesh, as lit_view has them: each with the id of its face, and a shading normal tilted from the face's"""
    (v, tr, fs, _), _ = scene(name)
    p, sn, fn = sr.points_on_faces(v, tr, 10, 5 + mode, tilt=0.3)
    ids = np.random.default_rng(5 + mode).integers(0, len(tr), 10)         # (the faces points_on_faces draws first)
    c = make_case(name, 10, 8, 3, 1, 16, 48, mode, seed=77 + mode, pts=p, nrm=sn)
    c["face"], c["face_nrm"] = ids.astype(np.int32), fn
    return c


def constant_case(name=0, P=3, N=128, L=(21.0, 32.5, 40.0), **kw):
    """mode 1, D = 1, a constant environment, no source: out = (2 pi L / N) sum of cos over the open paths, bit-equal to the emulation"""
    c = make_case(name, P, N, 1, 0, 1, 1, 1, sg=sv.sg_constant(L), bitexact=True, **kw)
    return c


TIE_SEED, TIE_POINT = 0x5EED0001, 2234025610


def tie_case():
    """One point, normal +z, no face, the constant environment, mode 1, D = 1, four paths in four lanes: out = (2 pi L / 4) sum of
    |w_z|.  The point's index in the call (point_base) was searched over all 2^32 counters at this seed for one whose four terms
    of channel 1 add up to two different binary32 numbers in the two orders: the lane-strided butterfly (t0 + t1) + (t2 + t3)
    gives 70.1582336, a serial sum ((t0 + t1) + t2) + t3 gives 70.158226.  The one output value shows the order of the sum"""
    return make_case(0, 1, 4, 1, 0, 1, 1, 1, sg=sv.sg_constant(), pts=[[0.1, 0.2, 0.3]], nrm=[[0.0, 0.0, 1.0]], seed_is=TIE_SEED,
                     point_base=TIE_POINT, bitexact=True)


def nan_case(mode):
    c = make_case("room", 5, 8, 2, 2, 16, 48, mode, seed=21)
    c["pts"][1, 0] = np.nan
    c["pts"][3] = np.nan
    if mode == 0:
        c["mat"] = sr.materials(5, c["pts"], 22)
    return c


SHAPE_N = (1, 2, 3, 64, 65, 200)
SHAPE_D = (1, 2, 4, 8)
SHAPE_S = (0, 1, 2, 5)
SHAPE_KP = (1, 16, 64)
SHAPE_J = (0, 1, 48, 64)
SHAPE_P = (1, 63, 64, 65)


def generic_cases():
    """name -> case: the cases of tests/test_gpu_surfpath.py through the C entry"""
    out = {}
    for i, N in enumerate(SHAPE_N):
        out[f"N={N}"] = make_case("window" if i % 2 else "room", 4, N, 2, 2, 16, 48, i % 2)
    for D in SHAPE_D:
        for mode in (0, 1):
            out[f"D={D} mode {mode}"] = make_case("window", 6, 16, D, 1, 16, 48, mode)
    for S in SHAPE_S:
        out[f"S={S}"] = make_case("room", 5, 16, 2, S, 16, 48, S % 2)
    for kp in SHAPE_KP:
        out[f"Kp={kp}"] = make_case("room", 5, 16, 2, 2, kp, 48, 0)
    for J in SHAPE_J:
        out[f"J={J}"] = make_case("window", 5, 17, 2, 1, 16, J, J % 2)
    for P in SHAPE_P:
        out[f"P={P}"] = make_case("room", P, 4, 2, 2, 16, 48, P % 2)
    for F in (0, 1):
        for mode in (0, 1):
            out[f"F={F} mode {mode}"] = make_case(F, 6, 17, 3, F, 1, 48, mode)
    for mode in (0, 1):
        out[f"on the mesh mode {mode}"] = on_mesh_case(mode)
        out[f"NaN points mode {mode}"] = nan_case(mode)
    out["point_base"] = make_case("window", 5, 16, 2, 1, 16, 48, 0, point_base=123457)
    out["point_base at the end"] = make_case("room", 5, 3, 2, 2, 16, 48, 1, point_base=2 ** 32 - 5)
    for N in (3, 128, 200):
        out[f"constant N={N}"] = constant_case(0, 3, N)
    out["constant in the room"] = constant_case("window", 6, 64)
    out["constant under the face"] = constant_case(1, 6, 16)
    out["tie"] = tie_case()
    return out


def mutant_case(mutant, fam):
    """the case a mutant is held against for the family `fam`: points on the mesh with tilted normals and their faces' ids, three
    segments, a source -- and what the mutant needs to show: paths that do not fill the lanes, a point_base, the planted tie"""
    mode = 1 if fam == "irradiance" else 0
    if mutant == "serial_sum":
        return tie_case()
    if mutant == "divide_by_padded":
        return make_case("window", 5, 3, 2, 1, 16, 48, mode)
    if mutant == "counter_without_point_base":
        return make_case("window", 5, 16, 2, 1, 16, 48, mode, point_base=123457)
    return on_mesh_case(mode)
