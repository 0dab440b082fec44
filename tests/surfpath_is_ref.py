"""Restatement of the importance-sampled path tracer on the surface (esr_nerf_amd/csrc/surfpath_is.hip, sources.path_light(
sampling="brdf") / lit_view / bake_irradiance(paths=)): section Y of include/esr_hip.h taken word by word in numpy and torch, with
none of the kernel's machinery; never imported by the product.  Scenes, Philox, the lane sum, the binary32 Disney reflection and
its error terms (lts_ref64.Q) are tests/surfpath_ref.py's.

  uniforms     the disc pair (the first candidate with 0 < s < 1 over the blocks 0 .. 7 of purpose 0) and the two words of purpose 2
  direction    the frame, the technique, the two samplers, the density: binary64 in the kernel's order
  lobe_cos     the lobe's inverse CDF alone (the host tests hold its histogram against the closed form)
  emulate      the kernel's ORDER of operations, as surfpath_ref.emulate: decisions from raycast_ref.brute's binary64 triangle test,
               binary32 interpolation, back-face test and BRDF, binary64 roulette, frame, samplers, density and sums.  Its mutants
               stand for the mistakes a sampler of this kind can make
  reference    the same quantity in float64 at the emulation's decisions, with `absref` from the error algebra lts_ref64.Q
  check        the checks of tests/test_gpu_surfpath_is.py on one case

Decisions and their bands (a path is `ambiguous`, and exempt from the equalities, when the restatement's value lies inside):
  u_t < q_s     both sides are correctly rounded binary64 operations on exact inputs: the kernel's bits; band |u_t - q_s| <= 2^-50
  disc test     likewise: |s - 1| <= 2^-50 or s <= 2^-50 at a candidate up to the one taken
  u_r >= q      q is the throughput's largest channel, which carries the binary32 reflections of the path so far:
                |u_r - q| <= 2 2^-24 E(q), E(q) the error algebra's bound on that channel (0 where q sits at a clamp, then 2^-50)
  oh <= 0       binary64 through log and exp (an ulp between libraries): |oh| <= 1e-9, and |oh'| <= 1e-9 for the lobe's draws
  cos <= 0      the flip-free hemisphere test, likewise: |cos| <= 1e-9
  hit / miss    raycast_ref.brute's `ambiguous`;  back face: the binary32 dot within FLIP_BAND of 0, as section X's

Bound.  |out - ref64| <= K_FAMILY[family] 2^-24 absref per value, on every point none of whose paths holds an ambiguous
decision.  absref is surfpath_ref's -- every rounding of every Disney chain of a path, of the interpolated normal and material
that enter it, the environment's lobes, section U's term, the binary64 sums' share, the final rounding -- with two additions.
The weight is R / P with P (2 pi times the density) a binary64 number: it scales the reflection's value and error alike.  The
roulette's division carries q's own error, E(T / q) = E(T) / q + |T| E(q) / q^2.  The conditioning of the lobe D is explicit in
the algebra: lts_ref64.xexp gives E(exp(a)) = exp(a) (E(a) + 2) and a = kappa (n.h - 1) has E(a) = kappa E(n.h) (+ roundings),
that is |dD / D| <= kappa |d(n.h)|.  Lobe sampling puts the samples where n.h -> 1 and D is largest, so this term is exercised at
full size: at roughness r the reflection's relative budget is about 4 kappa 2^-24 = 8 2^-24 / r^2.
MIN_ROUGH = 0.05 (kappa = 800, 8 2^-24 / r^2 = 1.9e-4) is the smallest roughness of the bounded cases: there absref still
separates a wrong weight from a right one (every mutant's error is a multiple of the value itself); at 0.01 the budget is 0.5 %
and below it the bound says nothing, so the case at roughness 0 (the 1e-7 clamp, kappa = 2e7) asserts `trace`, `end` and
finiteness only.  Wherever absref is not 0 it is raised by UNDERFLOW = 2^-100, binary32's absolute rounding floor 2^-126
magnified by at most 2^26: far off the mirror direction the lobe's exp underflows and no relative bound can hold.
"""
import math

import numpy as np
import torch

import lts_ref64 as lr
import raycast_ref as rr
import surfenv_ref as sv
import surflight_ref as sr
import surfpath_ref as sp
from surfpath_ref import COMPONENTS, INV2PI, U24, _T, _dot32, disney32, disney_q, family, philox, seed_key  # noqa: F401

FLIP_BAND = sp.FLIP_BAND
EXACT_BAND = 2.0 ** -50
DOUBLE_BAND = 1e-9
AMBIGUOUS_CAP = 0.001
MIN_ROUGH = 0.05
PI = math.pi
# binary32 rounds relatively only down to 2^-126: below it a result carries an absolute error of up to 2^-150 = 2^-24 2^-126 (the
# lobe's exp underflows far off the mirror direction at kappa = 800), which a path's throughput, the sources' geometry term and
# the radiance can magnify -- by no more than 2^26 in these scenes.  absref is this much larger wherever it is not 0
UNDERFLOW = 2.0 ** -100
# The worst |out - ref64| / (2^-24 absref) over every case of tests/test_gpu_surfpath_is.py (-s prints them) and, per family,
# the smallest power of two at or above the larger of the two.  MI355X / the emulation on the same cases:
#   env          0.092 / 0.215   (the GPU's worst on "point_base"; the emulation's on "P=64" as the GPU's host ran it -- 0.063 on
#                                another host: torch's binary32 exp differs by an ulp between CPUs, inside the algebra's 2 units)
#   src          0.123 / 0.151
#   irradiance   0.186 / 0.186   (the constant cases: the final binary32 rounding of a bit-equal value)
# Far under 1 for surfpath_ref's reasons: absref counts every rounding of every chain at full magnitude, and N paths average.
MEASURED = {"env": (0.092, 0.215), "src": (0.123, 0.151), "irradiance": (0.186, 0.186)}   # MI355X, emulation
K_FAMILY = {"env": 0.25, "src": 0.25, "irradiance": 0.25}

MUTANTS = ("no_4oh", "p_without_qs", "kappa_from_ro", "norm_2kappa", "no_mis", "T_not_divided", "rr_late", "frame_swapped",
           "cos_z_linear", "purpose_2b", "word_reused", "mode1_2pi_cos")


# ----------------------------------------------------------------------------------------------------------------------
# uniforms and the samplers


def uniforms(ctr0, sid, b, key, mutant=None):
    """-> dict(a1, a2, s f64 [m], found bool [m], ut, ur f64 [m], near bool [m]: a disc candidate up to the one taken within
    EXACT_BAND of the test's ends) for segment b of the paths (ctr0, sid)"""
    pw = (2 if mutant == "purpose_2b" else 4) * b
    m = len(ctr0)
    words = np.stack([philox(ctr0, sid, pw, blk, key) for blk in range(8)], -2) if m else np.zeros((0, 8, 4), np.uint32)
    a = (2.0 * (words.astype(np.float64) * 2.0 ** -32) - 1.0).reshape(m, 16, 2)
    s = a[:, :, 0] * a[:, :, 0] + a[:, :, 1] * a[:, :, 1]
    ok = (s > 0.0) & (s < 1.0)
    found = ok.any(1)
    first = np.where(found, ok.argmax(1), 15)
    rows = np.arange(m)
    near = ((np.abs(s - 1.0) <= EXACT_BAND) | (s <= EXACT_BAND)) & (np.arange(16)[None, :] <= first[:, None])
    r = philox(ctr0, sid, pw + 2, 0, key) if m else np.zeros((0, 4), np.uint32)
    ut = (r[:, 0].astype(np.float64) + 0.5) * 2.0 ** -32
    ur = ut if mutant == "word_reused" else (r[:, 1].astype(np.float64) + 0.5) * 2.0 ** -32
    z = lambda x: np.where(found, x, 0.0)
    return dict(a1=z(a[rows, first, 0]), a2=z(a[rows, first, 1]), s=z(s[rows, first]), found=found, ut=ut, ur=ur, near=near.any(1))


def kappa_of(rough, mutant=None):
    ro = np.asarray(rough, np.float32).astype(np.float64)
    return 2.0 / np.fmax(ro if mutant == "kappa_from_ro" else ro * ro, 1e-7)


def lobe_cos(s, kappa):
    """cos(theta) of the lobe's half vector for the uniform s in (0, 1]: the inverse of F(c) = (e^(kappa (c - 1)) - e^-kappa) / (1 - e^-kappa)"""
    with np.errstate(over="ignore"):
        ek = 1.0 / np.exp(kappa)
    return np.clip(1.0 + np.log(s + (1.0 - s) * ek) / kappa, 0.0, 1.0)


def lobe_cdf(c, kappa):
    return (np.exp(kappa * (c - 1.0)) - np.exp(-kappa)) / (1.0 - np.exp(-kappa))


def frame(nd, mutant=None):
    """(t1, t2) f64 [m, 3] of Duff et al. for the widened normals nd"""
    sg = np.copysign(1.0, nd[:, 2])
    with np.errstate(all="ignore"):
        a = -1.0 / (sg + nd[:, 2])
    b = (nd[:, 0] * nd[:, 1]) * a
    t1 = np.stack([1.0 + ((sg * nd[:, 0]) * nd[:, 0]) * a, sg * b, -(sg * nd[:, 0])], 1)
    t2 = np.stack([b, sg + (nd[:, 1] * nd[:, 1]) * a, -nd[:, 1]], 1)
    return (t2, t1) if mutant == "frame_swapped" else (t1, t2)


def technique(base, metal):
    """q_s f64 [m] of the widened material"""
    md = np.asarray(metal, np.float32).astype(np.float64)
    bs = np.asarray(base, np.float32).astype(np.float64)
    ab = ((bs[:, 0] + bs[:, 1]) + bs[:, 2]) / 3.0
    Fb, db = 0.04 * (1.0 - md) + ab * md, (1.0 - md) * ab
    sm = Fb + db
    with np.errstate(all="ignore"):
        r0 = Fb / sm
    qs = np.where(r0 >= 0.125, np.where(r0 <= 0.875, r0, 0.875), 0.125)
    return np.where(sm > 0.0, qs, 0.125)


def density2pi(nd, wod, w, qs, kappa, mutant=None):
    """P = 2 pi p of the directions w, cos = n . w and oh' = wo . h'"""
    with np.errstate(all="ignore"):
        ek = 1.0 / np.exp(kappa)
        cos = sr._dot(nd, w)
        hv = w + wod
        hl = np.sqrt((hv[:, 0] * hv[:, 0] + hv[:, 1] * hv[:, 1]) + hv[:, 2] * hv[:, 2])
        hv = hv / hl[:, None]
        nh = np.fmax(sr._dot(nd, hv), 0.0)
        ohp = sr._dot(wod, hv)
        norm = kappa / (1.0 - (ek * ek if mutant == "norm_2kappa" else ek))
        ps = norm * np.exp(kappa * (nh - 1.0))
        ps = ps if mutant == "no_4oh" else ps / (4.0 * ohp)
        ps = np.where(ohp > 0.0, ps, 0.0)
        if mutant == "p_without_qs":
            return ps + 2.0 * cos, cos, ohp
        if mutant == "no_mis":
            return 2.0 * cos, cos, ohp
        return qs * ps + (1.0 - qs) * (2.0 * cos), cos, ohp


def direction(n, wo, base, rough, metal, u, first_irr, mutant=None):
    """the direction of one segment at the vertices (n, wo, material: binary32 [m, .]) from the uniforms u -> dict(w f64 [m, 3],
    lobe bool, no_dir bool (code 4), P f64 (2 pi p), cos, near bool: a decision inside its band)"""
    m = len(n)
    nd, wod = np.asarray(n, np.float32).astype(np.float64), np.asarray(wo, np.float32).astype(np.float64)
    qs = np.zeros(m) if first_irr else technique(base, metal)
    lobe = u["ut"] < qs
    near = np.abs(u["ut"] - qs) <= EXACT_BAND
    kappa = kappa_of(rough, mutant)
    a1, a2, s = u["a1"], u["a2"], u["s"]
    with np.errstate(all="ignore"):
        sl = np.where(u["found"], s, 1.0)
        c = lobe_cos(sl, kappa)
        sn, rs = np.sqrt((1.0 - c) * (1.0 + c)), np.sqrt(sl)
        lx, ly, lz = np.where(lobe, (a1 * sn) / rs, a1), np.where(lobe, (a2 * sn) / rs, a2), np.where(lobe, c, (1.0 - s) if mutant == "cos_z_linear" else np.sqrt(1.0 - s))
        t1, t2 = frame(nd, mutant)
        h = (lx[:, None] * t1 + ly[:, None] * t2) + lz[:, None] * nd
        oh = sr._dot(wod, h)
        mv = (2.0 * oh)[:, None] * h - wod
        ln = np.sqrt((mv[:, 0] * mv[:, 0] + mv[:, 1] * mv[:, 1]) + mv[:, 2] * mv[:, 2])
        w = np.where(lobe[:, None], mv / ln[:, None], h)
        P, cos, ohp = density2pi(nd, wod, w, qs, kappa, mutant)
    no_dir = (lobe & ~(oh > 0.0)) | ~(cos > 0.0) | (lobe & ~(ohp > 0.0) & (not first_irr))
    near |= (lobe & ((np.abs(oh) <= DOUBLE_BAND) | (np.abs(ohp) <= DOUBLE_BAND))) | (np.abs(cos) <= DOUBLE_BAND)
    return dict(w=w, lobe=lobe, no_dir=no_dir, P=P, cos=cos, near=near, qs=qs)


# ----------------------------------------------------------------------------------------------------------------------
# the kernel's order of operations


def emulate(case, mutant=None):
    """-> dict(out f32 [P, 3, 3], n_open i32 [P], trace i32 [P, N, D], end u8 [P, N], ambiguous bool [P, N], terms f64 [P, N, 2, 3]
    (the paths' environment terms) and what `reference` replays) of a case of surfpath_ref.make_case with `rr` (rr_start; absent: D)"""
    v, tr, A, mode, N, D = case["v"], np.asarray(case["tr"], np.int64).reshape(-1, 3), case["attrs"], case["mode"], case["N"], case["D"]
    rr_start = case.get("rr", D)
    L, sg = case["L"], case["sg"]
    S, kp = (0, 1) if L is None else L["weight"].shape
    lgp = kp.bit_length() - 1
    J = 0 if sg is None else len(sg[0])
    pts, nrm = np.asarray(case["pts"], np.float64), np.asarray(case["nrm"], np.float32)
    P = len(pts)
    M = P * N
    f32 = np.float32
    pid, sid = np.repeat(np.arange(P), N), np.tile(np.arange(N), P)
    own = np.arange(P) if case.get("point_ids") is None else np.asarray(case["point_ids"], np.int64)
    ctr0 = case["point_base"] + own[pid]
    key = seed_key(case["seed"])
    x, n = pts[pid].copy(), nrm[pid].copy()
    if mode == 0:
        base, rough, metal, wo = (np.asarray(case["mat"][k], f32)[pid].copy() for k in ("base", "rough", "metal", "wo"))
    else:
        base, rough, metal, wo = np.zeros((M, 3), f32), np.zeros(M, f32), np.zeros(M, f32), np.zeros((M, 3), f32)
    base0, rough0, metal0 = base.copy(), rough.copy(), metal.copy()
    face = np.full(M, -1, np.int64) if case["face"] is None else np.asarray(case["face"], np.int64)[pid].copy()
    T = np.ones((M, 3))
    active = np.ones(M, bool)
    trace, end, amb, open0 = np.full((M, D), -2, np.int32), np.zeros(M, np.uint8), np.zeros(M, bool), np.zeros(M, bool)
    ev_env, ev_src = np.zeros((M, 2, 1, 3)), np.zeros((M, (D + 1) * max(S, 1), 3))
    exact = bool(case.get("exact"))
    segs = []
    cast = np.zeros(M, np.int64)
    pw = 2 if mutant == "purpose_2b" else 4

    def nee(idx, b, event0):
        rec = []
        for s in range(S):
            word = philox(ctr0[idx], sid[idx], pw * b + 1, s >> 2, key)[:, s & 3]
            k = (word >> np.uint32(32 - lgp)).astype(np.int64) if lgp else np.zeros(len(idx), np.int64)
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
            cast[idx[li]] += 1
            if not exact:
                amb[idx[li]] |= br["ambiguous"]
            vi = li[~br["hit"]]
            if not len(vi):
                continue
            q = idx[vi]
            wl = ws[vi].astype(f32)
            R = disney32(base[q], rough[q], metal[q], n[q], wl, wo[q]).astype(np.float64)
            term = ((R * INV2PI) * G[vi][:, None]) * E[vi]
            ev_src[q, event0 + s] = T[q] * (float(kp) * term)
            rec.append(dict(q=q, wl=wl, c=(INV2PI * G[vi])[:, None] * E[vi], event=event0 + s))
        return rec

    for b in range(D):
        act = np.flatnonzero(active)
        if not len(act):
            break
        u = uniforms(ctr0[act], sid[act], b, key, mutant)
        if not exact:
            amb[act] |= u["near"]
        seg = dict(b=b, rr=None, nee=[])
        if b >= rr_start + (1 if mutant == "rr_late" else 0):
            with np.errstate(all="ignore"):
                mx = np.fmax(np.fmax(T[act, 0], T[act, 1]), T[act, 2])
                q = np.where(mx >= 0.0625, np.where(mx <= 1.0, mx, 1.0), 0.0625)
                q = np.where(np.isnan(mx), 1.0, q)
                die = u["ur"] >= q
                if mutant != "T_not_divided":
                    T[act] = T[act] / q[:, None]
            seg["rr"] = dict(idx=act, q=q, ur=u["ur"], free=(mx > 0.0625) & (mx < 1.0), arg=np.argmax(np.nan_to_num(T[act], nan=-np.inf), 1))
            end[act[die]], active[act[die]] = 3, False
            keep = ~die
            act, u = act[keep], {k: a[keep] for k, a in u.items()}
        first_irr = mode == 1 and b == 0
        dr = direction(n[act], wo[act], base[act], rough[act], metal[act], u, first_irr, mutant)
        if not exact:
            amb[act] |= dr["near"]
        gone = dr["no_dir"]
        end[act[gone]], active[act[gone]] = 4, False
        idx, w, Pd = act[~gone], dr["w"][~gone], dr["P"][~gone]
        wi = w.astype(f32)
        if first_irr:
            Wt = np.full((len(idx), 3), PI)
            if mutant == "mode1_2pi_cos":
                Wt = np.repeat((dr["cos"][~gone] * (2.0 * PI))[:, None], 3, 1)
            scale = np.ones(len(idx))
        else:
            with np.errstate(all="ignore"):
                scale = 1.0 / Pd
                Wt = disney32(base[idx], rough[idx], metal[idx], n[idx], wi, wo[idx]).astype(np.float64) / Pd[:, None]
        with np.errstate(all="ignore"):
            T[idx] = T[idx] * Wt
        br = rr.brute(v, tr, x[idx], w, case["t_min"], np.inf, face[idx])
        cast[idx[np.isfinite(x[idx]).all(1)]] += 1
        if not exact:
            amb[idx] |= br["ambiguous"]
        hit = br["hit"]
        trace[idx, b] = np.where(hit, br["face"], -1)
        mi = idx[~hit]
        comp = 0 if b == 0 else 1
        if J and len(mi):
            Lenv = sv.env32(sg, wi[~hit]).astype(np.float64)
            with np.errstate(all="ignore"):
                ev_env[mi, comp, 0] = T[mi] * Lenv
        if b == 0:
            open0[mi] = True
        end[mi], active[mi] = 1, False
        seg.update(idx=idx, wi=wi, irr=first_irr, Wt=Wt, scale=scale, miss=mi, miss_wi=wi[~hit], comp=comp, lobe=dr["lobe"][~gone])
        hi = idx[hit]
        if len(hi):
            f, uu, vv = br["face"][hit], br["u"][hit], br["v"][hit]
            wts = np.stack([(1.0 - uu) - vv, uu, vv], 1)
            ids = tr[f]
            xn = (wts[:, 0:1] * v[ids[:, 0]] + wts[:, 1:2] * v[ids[:, 1]]) + wts[:, 2:3] * v[ids[:, 2]]
            w32 = wts.astype(f32)
            at = lambda a: (w32[:, 0:1] * a[ids[:, 0]] + w32[:, 1:2] * a[ids[:, 1]]) + w32[:, 2:3] * a[ids[:, 2]]
            nn = at(np.asarray(A["normal"], f32))
            with np.errstate(all="ignore"):
                ln = np.sqrt((nn[:, 0] * nn[:, 0] + nn[:, 1] * nn[:, 1]) + nn[:, 2] * nn[:, 2])
                ok = (ln > 0) & np.isfinite(ln)
                n_new = nn / ln[:, None]
                wo_new = -wi[hit]
                dt = _dot32(n_new, wo_new)
                alive = ok & (dt > 0)
            if not exact:
                amb[hi] |= ok & (np.abs(dt) <= f32(FLIP_BAND))
            dead, go = hi[~alive], hi[alive]
            end[dead], active[dead] = 2, False
            x[go], n[go], wo[go], face[go] = xn[alive], n_new[alive], wo_new[alive], f[alive]
            base[go], rough[go], metal[go] = at(np.asarray(A["base"], f32))[alive], at(np.asarray(A["rough"], f32)[:, None])[alive, 0], \
                at(np.asarray(A["metal"], f32)[:, None])[alive, 0]
            seg.update(go=go, ids=ids[alive], wts=wts[alive])
            if S and len(go):
                seg["nee"] = nee(go, b, (b + 1) * S)
        segs.append(seg)
    sh = lambda a: a.reshape((P, N) + a.shape[1:])
    with np.errstate(all="ignore"):
        sums = np.stack([sp._lane_sum(sh(ev_env[:, 0]), N), sp._lane_sum(sh(ev_env[:, 1]), N), sp._lane_sum(sh(ev_src), N)], 1)
        out = (sums / float(N)).astype(f32)
    if not J:
        out[:, :2] = 0.0
    return dict(out=out, n_open=sh(open0).sum(1).astype(np.int32), trace=sh(trace), end=sh(end), ambiguous=sh(amb), segs=segs,
                terms=sh(ev_env[:, :, 0]), src_terms=sh(ev_src).sum(2), base0=base0, rough0=rough0, metal0=metal0, cast=sh(cast))


def reference(case, emu):
    """(value f64 [P, 3, 3], absref [P, 3, 3], near bool [P, N]: a roulette decision inside its band) at the emulation's decisions"""
    A, mode, N, L, sg = case["attrs"], case["mode"], case["N"], case["L"], case["sg"]
    P = len(case["pts"])
    M = P * N
    kp = 1 if L is None else L["weight"].shape[1]
    if not M:
        return np.zeros((P, 3, 3)), np.zeros((P, 3, 3)), np.zeros((P, N), bool)
    Q = lr.Q
    pid = np.repeat(np.arange(P), N)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    st = {k: [_T(np.asarray(a, np.float64)), z(*a.shape)] for k, a in
          (("n", np.asarray(case["nrm"], np.float32)[pid]), ("base", emu["base0"]), ("rough", emu["rough0"]), ("metal", emu["metal0"]))}
    wo = np.zeros((M, 3), np.float32) if mode == 1 else np.asarray(case["mat"]["wo"], np.float32)[pid].copy()
    Tv, TE = np.ones((M, 3)), np.zeros((M, 3))
    val, err, mag = np.zeros((M, 3, 3)), np.zeros((M, 3, 3)), np.zeros((M, 3, 3))
    near = np.zeros(M, bool)
    get = lambda k, q: Q(st[k][0][q], st[k][1][q])
    for seg in emu["segs"]:
        if seg["rr"] is not None:
            r = seg["rr"]
            a, q = r["idx"], r["q"]
            rows = np.arange(len(a))
            qE = np.where(r["free"], TE[a][rows, r["arg"]], 0.0)
            near[a] |= np.abs(r["ur"] - q) <= 2.0 * U24 * qE + EXACT_BAND
            TE[a] = TE[a] / q[:, None] + np.abs(Tv[a]) * (qE / (q * q))[:, None]
            Tv[a] = Tv[a] / q[:, None]
        idx, wi = seg["idx"], seg["wi"]
        if seg["irr"]:
            Rv, RE = np.full((len(idx), 3), PI), np.zeros((len(idx), 3))
        else:
            Rv, RE = disney_q(get("base", idx), get("rough", idx), get("metal", idx), get("n", idx), wi, wo[idx])
            # (1 / P is binary64: it scales value and error alike; its own 2^-53 is inside the sums' 64 2^-29 share below)
            Rv, RE = Rv * seg["scale"][:, None], RE * seg["scale"][:, None]
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
    absref = (sh(err).sum(1) + 64 * 2.0 ** -29 * sh(mag).sum(1)) / N + np.abs(value)
    return value, absref, near.reshape(P, N)


def check(case, out, n_open=None, trace=None, end=None, emu=None, what="", families=None, values=True):
    """The GPU's checks of one case -> (worst ratio per family, ambiguous paths); raises AssertionError.  `values=False`: only
    trace, end, n_open and finiteness (the case at roughness 0)"""
    emu = emu or emulate(case)
    out = np.asarray(out)
    assert out.dtype == np.float32 and out.shape == emu["out"].shape, (what, out.dtype, out.shape)
    if "ref" not in emu:
        emu["ref"] = reference(case, emu)
    value, absref, near = emu["ref"]
    amb = emu["ambiguous"] | near
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
    if not values:
        assert np.isfinite(out[clear]).all(), (what, "not finite")
        return {}, int(amb.sum())
    if case.get("bitexact"):
        bad = np.argwhere((out.view(np.uint32) != emu["out"].view(np.uint32)).any((1, 2)) & clear)
        assert len(bad) == 0, (what, "not bit-equal to the emulation", out[bad[:2, 0]].tolist(), emu["out"][bad[:2, 0]].tolist())
    err = np.abs(out.astype(np.float64) - value)
    absref = np.where(absref > 0, absref + UNDERFLOW, 0.0)
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
# scenes and cases


_attrs = {}


def attrs_is(name, kind="span"):
    """surfpath_ref's per-vertex attributes of a scene with another roughness: "span" 1.0 down to MIN_ROUGH (both ends are
    taken), "zero" 0 everywhere, "diffuse" (rough 1, metal 0) and "glossy" (rough 0.1, metal 1) for the variance cases"""
    if kind == "plain":
        return sp.scene(name)[1]
    if (name, kind) not in _attrs:
        a = dict(sp.scene(name)[1])
        V = len(a["rough"])
        rng = np.random.default_rng(900 + V)
        if kind == "span":
            ro = np.exp(rng.uniform(math.log(MIN_ROUGH), 0.0, V))
            ro[::7], ro[3::7] = MIN_ROUGH, 1.0
            a["rough"] = ro.astype(np.float32)
        elif kind == "zero":
            a["rough"] = np.zeros(V, np.float32)
        elif kind == "black":
            a["base"] = np.zeros((V, 3), np.float32)
        else:
            a["rough"] = np.full(V, 1.0 if kind == "diffuse" else 0.1, np.float32)
            a["metal"] = np.full(V, 0.0 if kind == "diffuse" else 1.0, np.float32)
        _attrs[(name, kind)] = a
    return _attrs[(name, kind)]


def make_case(name="room", P=5, N=16, D=2, S=2, kp=16, J=48, mode=0, rr=None, kind="span", seed=None, **kw):
    """surfpath_ref.make_case with the roughness of `kind` at the vertices and, in mode 0, at the points, and rr_start `rr`"""
    c = sp.make_case(name, P, N, D, S, kp, J, mode, seed=seed, **kw)
    c["attrs"] = attrs_is(name, kind)
    c["rr"] = D if rr is None else rr
    if mode == 0:
        m = dict(c["mat"])
        n_p = len(m["rough"])
        rng = np.random.default_rng(77 + n_p + N + D)
        if kind == "span":
            m["rough"] = np.exp(rng.uniform(math.log(MIN_ROUGH), 0.0, n_p)).astype(np.float32)
            m["rough"][::3] = MIN_ROUGH
            m["rough"][1::5] = 1.0
        elif kind == "zero":
            m["rough"] = np.zeros(n_p, np.float32)
        elif kind == "black":
            m["base"] = np.zeros((n_p, 3), np.float32)
        elif kind in ("diffuse", "glossy"):
            m["rough"] = np.full(n_p, 1.0 if kind == "diffuse" else 0.1, np.float32)
            m["metal"] = np.full(n_p, 0.0 if kind == "diffuse" else 1.0, np.float32)
        c["mat"] = m
    return c


def on_mesh_case(mode, rr=1, kind="span"):
    c = sp.on_mesh_case(mode)
    c["attrs"], c["rr"] = attrs_is("window", kind), rr
    if mode == 0:
        m = dict(c["mat"])
        m["rough"] = np.array([0.05, 1.0, 0.3, 0.9, 0.1, 0.5, 0.05, 0.7, 0.2, 1.0], np.float32)
        c["mat"] = m
    return c


def constant_case(name=0, P=3, N=128, L=(21.0, 32.5, 40.0), **kw):
    """mode 1, D = 1, a constant environment, no source: every open path adds pi L exactly, out = pi L n_open / N, bit-equal"""
    c = sp.constant_case(name, P, N, L, **kw)
    c["rr"] = 1
    return c


def room_stat_case(kind, copies, D=3, S=0, rr_start=None, seed=3):
    """the box room of tests/test_surfpath_host.py (raycast_ref.room_points, the tilted normal, 48 lobes) with the material `kind`
    at the points and at the vertices: `copies` copies of the 8 points with ONE path each, so that out[p] is the path's own value
    in all three components (the copies differ in the counter's point word); copy j of point i is row 8 j + i"""
    pts = np.tile(rr.room_points(), (copies, 1))
    nrm = sr.unit32(np.tile([[0.1, -0.2, 1.0]], (len(pts), 1)))
    c = make_case("room", len(pts), 1, D, S, 16 if S else 1, 48, 0, rr=rr_start, kind=kind, seed=seed, pts=pts, nrm=nrm, t_min=1e-6)
    if "mat" in c:                                                          # (the same material at every copy of a point)
        c["mat"] = {k: np.tile(a[:8], (copies,) + (1,) * (a.ndim - 1)) for k, a in c["mat"].items()}
    return c


def grazing_case():
    """wo at the first vertex grazing (n . wo = 1e-3) and below the horizon (n . wo < 0): the lobe's mirror direction leaves the
    hemisphere often (code 4), the cosine technique never"""
    c = make_case("window", 6, 32, 2, 1, 16, 48, 0, rr=1, seed=91)
    wo = c["mat"]["wo"].copy()
    n = c["nrm"].astype(np.float64)
    t = np.cross(n, [0.3, 0.5, 0.8])
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    wo[:3] = sr.unit32(t[:3] + 1e-3 * n[:3])
    wo[3:] = sr.unit32(t[3:] - 0.2 * n[3:])
    c["mat"] = dict(c["mat"], wo=wo, metal=np.ones(6, np.float32), rough=np.full(6, 0.3, np.float32))
    return c


def sphere_case(mode):
    """a sphere of 3 216 faces around the points: a closed cavity with smooth normals"""
    if "sphere" not in _attrs:
        v, tr = _sphere()
        _attrs["sphere"] = (v, tr)
    v, tr = _attrs["sphere"]
    rng = np.random.default_rng(12)
    V = len(v)
    attrs = dict(normal=sr.unit32(-v), base=rng.uniform(0.1, 0.9, (V, 3)).astype(np.float32),
                 rough=np.exp(rng.uniform(math.log(MIN_ROUGH), 0.0, V)).astype(np.float32), metal=rng.uniform(0, 1, V).astype(np.float32))
    P = 4
    pts = rng.uniform(-0.4, 0.4, (P, 3))
    nrm = sr.unit32(rng.uniform(-1, 1, (P, 3)))
    c = dict(v=v, tr=tr, attrs=attrs, L=None, sg=sv.sg_random(48, 5), pts=pts, nrm=nrm, face=None, mode=mode, N=16, D=3, t_min=1e-6, eps=1e-3,
             seed=0x51CE ^ mode, point_base=0, face_nrm=nrm.copy(), scene="sphere", rr=2)
    if mode == 0:
        c["mat"] = sr.materials(P, pts, 13, eye=(0.0, 0.0, 0.0))
    return c


def _sphere(n_lat=68, n_lon=24):
    """a latitude-longitude unit sphere of 2 n_lon (n_lat - 1) faces: 3 216 for 67 rings of 24 vertices"""
    v = [[0.0, 0.0, 1.0]]
    for i in range(1, n_lat):
        th = math.pi * i / n_lat
        for j in range(n_lon):
            ph = 2.0 * math.pi * j / n_lon
            v.append([math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)])
    v.append([0.0, 0.0, -1.0])
    tr = []
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    for j in range(n_lon):
        tr.append((0, ring(1, j), ring(1, j + 1)))
        tr.append((len(v) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            tr.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            tr.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    return np.array(v, np.float64), np.array(tr, np.int64)


SHAPE_N = (1, 2, 3, 64, 65, 200)
SHAPE_D = (1, 2, 3, 4, 5, 6, 7, 8)
SHAPE_P = (1, 63, 64, 65)


def generic_cases():
    """name -> case: the cases of tests/test_gpu_surfpath_is.py through the C entry"""
    out = {}
    for i, N in enumerate(SHAPE_N):
        out[f"N={N}"] = make_case("window" if i % 2 else "room", 4, N, 2, 2, 16, 48, i % 2, rr=1 + i % 2)
    for D in SHAPE_D:
        out[f"D={D}"] = make_case("window", 4, 8, D, 1, 16, 48, D % 2, rr=(1, 2, D)[D % 3])
    for rr_start in (1, 2, 4):
        for mode in (0, 1):
            out[f"rr_start={rr_start} mode {mode}"] = make_case("window", 6, 16, 4, 1, 16, 48, mode, rr=rr_start)
    for S in (0, 1, 2):
        out[f"S={S}"] = make_case("room", 5, 16, 2, S, 16, 48, S % 2, rr=1)
    for kp in (1, 16):
        out[f"Kp={kp}"] = make_case("room", 5, 16, 2, 2, kp, 48, 0, rr=2)
    for J in (0, 48):
        out[f"J={J}"] = make_case("window", 5, 17, 2, 1, 16, J, J % 2 if J else 0, rr=1)
    for P in SHAPE_P:
        out[f"P={P}"] = make_case("room", P, 4, 2, 2, 16, 48, P % 2, rr=1)
    for F in (0, 1):
        for mode in (0, 1):
            out[f"F={F} mode {mode}"] = make_case(F, 6, 17, 3, F, 1, 48, mode, rr=1)
    for mode in (0, 1):
        out[f"sphere mode {mode}"] = sphere_case(mode)
        out[f"on the mesh mode {mode}"] = on_mesh_case(mode)
        c = make_case("room", 5, 8, 2, 2, 16, 48, mode, rr=1, seed=21)
        c["pts"][1, 0] = np.nan
        c["pts"][3] = np.nan
        out[f"NaN points mode {mode}"] = c
    for metal in (0.0, 1.0):
        c = make_case("window", 5, 16, 3, 1, 16, 48, 0, rr=2, seed=300 + int(metal))
        c["mat"] = dict(c["mat"], metal=np.full(5, metal, np.float32))
        c["attrs"] = dict(c["attrs"], metal=np.full(len(c["attrs"]["metal"]), metal, np.float32))
        out[f"metallic {int(metal)}"] = c
    out["black base colour"] = make_case("window", 5, 16, 3, 1, 16, 48, 0, rr=2, kind="black", seed=310)
    out["grazing wo"] = grazing_case()
    out["point_base"] = make_case("window", 5, 16, 2, 1, 16, 48, 0, rr=1, point_base=123457)
    out["point_base at the end"] = make_case("room", 5, 3, 2, 2, 16, 48, 1, rr=1, point_base=2 ** 32 - 5)
    for N in (3, 128):
        out[f"constant N={N}"] = constant_case(0, 3, N)
    out["constant in the room"] = constant_case("window", 6, 64)
    return out


def zero_rough_case():
    """roughness 0 everywhere: kappa = 2e7 at the 1e-7 clamp.  No roulette: there the throughput's binary32 reflection is
    conditioned by kappa 2^-24 > 1, so a decision taken from it is no decision; the directions are binary64 and stay comparable"""
    return make_case("window", 6, 16, 3, 1, 16, 48, 0, rr=None, kind="zero", seed=55)


def mutant_case(mutant):
    """the small case a mutant is held against: points on the mesh with tilted normals, three segments, a source, the roulette
    from segment 1 on, roughness from MIN_ROUGH to 1 -- mode 1 for the mutant of mode 1's first weight"""
    if mutant == "mode1_2pi_cos":
        return on_mesh_case(1)
    if mutant == "norm_2kappa":
        c = on_mesh_case(0)                                                 # (e^-kappa is visible only under a wide lobe)
        c["mat"] = dict(c["mat"], rough=np.full(10, 1.0, np.float32), metal=np.full(10, 1.0, np.float32))
        return c
    return on_mesh_case(0)
