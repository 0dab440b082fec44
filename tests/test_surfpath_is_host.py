"""The importance-sampled path tracer without a GPU: the header's entry against the binding, the refusals of the Python layer
(raised before anything is launched), the keys of lit_view / bake_irradiance with and without the new keywords, the two samplers
against their closed forms, the density's integral, the restatement (tests/surfpath_is_ref.py) against surfpath_ref's uniform
estimator -- the same mean, a smaller variance -- the roulette's mean, the emulation inside every check the GPU has to pass with
no ambiguous decision, and its mutants outside.

The tests of the entry, the Python layer and (in test_surfpath_is_isa.py, test_gpu_surfpath_is.py) the kernel need the product's
new code.  The sampler, density, mean, variance and mutant tests exercise tests/surfpath_is_ref.py alone: they hold the
restatement against closed forms and against surfpath_ref's uniform estimator, and the kernel is then held against the
restatement on the GPU -- without the product's change they lack nothing but this file and the restatement."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import raycast_ref as rr
import surfenv_ref as sv
import surflight_ref as sr
import surfpath_is_ref as si
import surfpath_ref as sp
from conftest import ROOT

KEY = sp.seed_key(0xC0FFEE1234)


def test_the_entry_is_the_headers():
    import ctypes as C
    from esr_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    proto = re.search(r"\nint esr_surface_path_is\(([^)]*)\);", header).group(1)
    params = [" ".join(p.split()) for p in proto.split(",")]
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    want = [C.c_void_p if "*" in p else kinds[p.rsplit(" ", 1)[0]] for p in params]
    assert len(params) == 41 and _lib.SIGNATURES["esr_surface_path_is"] == (C.c_int, want) and "esr_surface_path_is" in _lib.EXPORTS
    names = [p.replace("*", " ").split()[-1] for p in params]
    old = [p.replace("*", " ").split()[-1] for p in re.search(r"\nint esr_surface_path\(([^)]*)\);", header).group(1).split(",")]
    assert [x for x in names if x != "rr_start"] == old and names[names.index("rr_start") - 1] == "depth"
    assert params[names.index("rr_start")] == "int32_t rr_start"
    assert _lib.ABI_VERSION == int(re.search(r"#define ESR_ABI_VERSION (\d+)", header).group(1)) >= 48
    assert re.search(r"\n \* Y\. Importance-sampled path-traced light on the surface", header)
    src = open(os.path.join(ROOT, "esr_nerf_amd", "csrc", "surfpath_is.hip")).read()
    assert all(f'#include "{h}"' in src for h in ("bvh_walk.h", "disney.h", "sg_env.h"))


def _cpu_surface():
    from esr_nerf_amd import sources
    v, tr, fs, S = rr.room()
    V = len(v)
    attrs = dict(normal=torch.zeros(V, 3), basecolor=torch.zeros(V, 3), roughness=torch.zeros(V), metallic=torch.zeros(V),
                 emission=torch.zeros(V, 3))
    z3, z1 = torch.zeros(0, 3, dtype=torch.float64), torch.zeros(0, dtype=torch.float64)
    rep = sources.SourceReport(0.1, torch.zeros(len(tr), dtype=torch.int32) - 1, torch.zeros(0, dtype=torch.int64), z1, z3, z3, z3, z3, z1.float(), z3, z3)
    return sources.Surface(torch.from_numpy(v), torch.from_numpy(tr), attrs), rep


BAD_SAMPLING = [dict(sampling="cosine"), dict(sampling=None), dict(sampling=1), dict(roulette=1), dict(sampling="uniform", roulette=2),
                dict(sampling="brdf", roulette=0), dict(sampling="brdf", roulette=-1), dict(sampling="brdf", roulette=True),
                dict(sampling="brdf", roulette=1.0), dict(sampling="brdf", roulette="2"), dict(sampling="brdf", roulette=2 ** 31)]


def test_python_layer_refuses_bad_inputs_before_any_launch(monkeypatch):
    from esr_nerf_amd import _lib, sources
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("a launch"))
    surf, rep = _cpu_surface()
    P = 5
    pts, nrm = torch.zeros(P, 3, dtype=torch.float64), torch.zeros(P, 3)
    env = tuple(torch.from_numpy(x) for x in sv.sg_random(48, 0))
    mat = dict(basecolor=nrm, roughness=nrm[:, 0], metallic=nrm[:, 0], wo=nrm)
    for kw in BAD_SAMPLING + [dict(sampling="brdf", paths=0), dict(sampling="brdf", depth=9), dict(sampling="brdf", seed=-1)]:
        with pytest.raises(ValueError):
            sources.path_light(surf, rep, points=pts, normals=nrm, env=env, **mat, **kw)
    # the roulette may start past the depth (it never runs then), and sampling alone is enough
    assert sources._path_sampling("x", "brdf", None, 3) == 3 and sources._path_sampling("x", "brdf", 7, 3) == 7
    assert sources._path_sampling("x", "brdf", 1, 3) == 1 and sources._path_sampling("x", "uniform", None, 3) is None


def _no_face_view(monkeypatch):
    from esr_nerf_amd import raycast, sources
    H, W = 3, 4
    N = H * W
    monkeypatch.setattr(raycast, "build", lambda v, t: "bvh")
    monkeypatch.setattr(raycast, "pixel_rays", lambda cams, view: (torch.zeros(N, 3, dtype=torch.float64), torch.ones(N, 3, dtype=torch.float64), None))
    monkeypatch.setattr(raycast, "cast", lambda bvh, o, d: types.SimpleNamespace(
        face=torch.full((N,), -1, dtype=torch.int32), t=torch.full((N,), float("inf"), dtype=torch.float64), bary=torch.zeros(N, 2, dtype=torch.float64)))
    surf = sources.Surface(torch.zeros(3, 3, dtype=torch.float64), torch.zeros(0, 3, dtype=torch.int64), {"emission": torch.zeros(3, 3)})
    z3, z1 = torch.zeros(0, 3, dtype=torch.float64), torch.zeros(0, dtype=torch.float64)
    rep = sources.SourceReport(0.1, torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int64), z1, z3, z3, z3, z3, z1.float(), z3, z3)
    return surf, rep, types.SimpleNamespace(n_views=1, device=torch.device("cpu"), width=W, height=H)


def test_lit_view_passes_the_keywords_and_keeps_its_keys_without(monkeypatch):
    from esr_nerf_amd import sources
    surf, rep, cams = _no_face_view(monkeypatch)
    plain = sources.lit_view(surf, rep, cams, 0)
    assert set(plain) == {"lin/reflect", "lin/emit", "face", "depth"}
    uniform = sources.lit_view(surf, rep, cams, 0, paths=4, depth=2, seed=3)
    for kw in (dict(sampling="brdf"), dict(sampling="brdf", roulette=1), dict(sampling="brdf", roulette=5), dict(sampling="uniform")):
        traced = sources.lit_view(surf, rep, cams, 0, paths=4, depth=2, seed=3, **kw)
        assert set(traced) == set(uniform) == set(plain) | {"lin/env_dir", "lin/env_indir", "lin/src_indir", "etc/open"}
        for k in plain:
            assert torch.equal(plain[k], traced[k]), k
    for kw in BAD_SAMPLING:
        with pytest.raises(ValueError):
            sources.lit_view(surf, rep, cams, 0, paths=4, **kw)
    for kw in (dict(sampling="brdf"), dict(roulette=2), dict(sampling="brdf", roulette=2)):
        with pytest.raises(ValueError):
            sources.lit_view(surf, rep, cams, 0, **kw)                      # (they are the paths')
    import inspect
    for fn in (sources.lit_view, sources.path_light):
        sig = inspect.signature(fn).parameters
        assert sig["sampling"].default == "uniform" and sig["roulette"].default is None


def test_bake_irradiance_takes_paths_and_keeps_its_keys_without(monkeypatch):
    """the launches replaced: what bake_irradiance asks of path_light, and the keys with and without `paths`"""
    from esr_nerf_amd import raycast, sources
    W, S = 4, 2
    face = torch.full((W, W), -1, dtype=torch.int32)
    face[1, :3] = torch.tensor([5, 6, 7], dtype=torch.int32)
    flags = (face >= 0).to(torch.uint8)
    flags[1, 2] = 0                                                         # (an owned texel whose centre is outside its face)
    atlas = types.SimpleNamespace(size=W, face=face, flags=flags, point=torch.arange(W * W * 3, dtype=torch.float32).reshape(W, W, 3))
    surf = types.SimpleNamespace(vertices=torch.zeros(3, 3, dtype=torch.float64), triangles=torch.zeros(8, 3, dtype=torch.int64))
    calls = []

    class Rep:
        def __len__(self):
            return S

    def path_light(surface, report, points, normals, faces, **kw):
        calls.append(dict(kw, points=points, faces=faces))
        n = points.shape[0]
        return {k: torch.full((n, 3), float(i + 1)) for i, k in enumerate(sp.COMPONENTS)}
    monkeypatch.setattr(sources, "_check_atlas", lambda *a: None)
    monkeypatch.setattr(raycast, "build", lambda v, t: "bvh")
    monkeypatch.setattr(sources, "source_lights", lambda *a: "lights")
    monkeypatch.setattr(sources, "face_normals", lambda s: torch.ones(8, 3))
    monkeypatch.setattr(sources, "direct_light", lambda surface, lights, p, n, **kw: torch.ones(p.shape[0], S, 3))
    monkeypatch.setattr(sources, "path_light", path_light)
    plain = sources.bake_irradiance(surf, atlas, Rep())
    assert set(plain) == {"light/sources"} and not calls
    baked = sources.bake_irradiance(surf, atlas, Rep(), paths=8, depth=3, seed=5, roulette=2, chunk=1)
    assert set(baked) == {"light/sources", "light/paths"} and torch.equal(baked["light/sources"], plain["light/sources"])
    lp = baked["light/paths"]
    assert lp.dtype == torch.float32 and tuple(lp.shape) == (W, W, 3, 3)
    assert torch.equal(lp[1, :2], torch.tensor([1.0, 2.0, 3.0])[None, :, None].expand(2, 3, 3)) and float(lp.sum()) == 2 * 18.0
    (c,) = calls
    assert c["mode"] == 1 and c["sampling"] == "brdf" and c["roulette"] == 2 and c["paths"] == 8 and c["depth"] == 3 and c["seed"] == 5
    assert c["faces"].tolist() == [5, 6] and c["env"] is None and c["lights"] == "lights" and c["bvh"] == "bvh"
    assert c["points"].dtype == torch.float64 and torch.equal(c["points"], atlas.point[1, :2].double())
    for kw in (dict(paths=0), dict(paths=4097), dict(paths=True), dict(paths=4, depth=0), dict(paths=4, depth=9), dict(paths=4, seed=-1),
               dict(paths=4, roulette=0), dict(paths=4, roulette=1.5), dict(roulette=2)):
        with pytest.raises(ValueError):
            sources.bake_irradiance(surf, atlas, Rep(), **kw)
    assert len(calls) == 1


# ----------------------------------------------------------------------------------------------------------------------
# the samplers and the density


@pytest.fixture(scope="module")
def draws():
    n = 1 << 20
    u = si.uniforms(np.arange(n), np.full(n, 7), 2, KEY)
    assert u["found"].all() and (u["s"] > 0).all() and (u["s"] < 1).all() and (u["ut"] > 0).all() and (u["ut"] < 1).all() and not u["near"].any()
    return u


@pytest.mark.parametrize("rough", [1.0, 0.2, 0.05])
def test_the_lobe_sampler_follows_its_cdf(draws, rough):
    """cos(theta) of 2^20 half vectors in 32 bins of equal probability under the closed-form CDF F(c) = (e^(kappa (c - 1)) -
    e^-kappa) / (1 - e^-kappa): chi^2 with 31 degrees of freedom (61.1 is the 1e-3 quantile), and the first moment of e^(kappa
    (c - 1)), whose mean under the lobe is (1 + e^-kappa) / 2"""
    kappa = float(si.kappa_of(np.float32(rough)))
    c = si.lobe_cos(draws["s"], kappa)
    n = len(c)
    assert (c >= 0).all() and (c <= 1).all()
    edges_c = np.zeros(33)                                                  # F^-1 of the bin edges
    edges_c[1:] = 1.0 + np.log(np.linspace(0, 1, 33)[1:] * (1 - math.exp(-kappa)) + math.exp(-kappa)) / kappa
    assert np.allclose(si.lobe_cdf(edges_c, kappa), np.linspace(0, 1, 33), atol=1e-12)
    bins = np.histogram(c, bins=edges_c)[0]
    chi2 = float(((bins - n / 32) ** 2 / (n / 32)).sum())
    e = np.exp(kappa * (c - 1.0))
    lo = math.exp(-kappa)
    want, var = (1 + lo) / 2, (1 - lo) ** 2 / 12
    print(f"kappa {kappa:.1f}: chi^2 {chi2:.1f}, E e^(kappa (c - 1)) {e.mean():.6f} (closed form {want:.6f})")
    assert bins.sum() == n and chi2 < 61.1, chi2
    assert abs(e.mean() - want) <= 5 * math.sqrt(var / n)
    # the azimuth is the pair's: uniform over 16 bins, and independent of s (the two halves of s give the same histogram)
    phi = np.arctan2(draws["a2"], draws["a1"])
    for half in (draws["s"] < 0.5, draws["s"] >= 0.5):
        m = int(half.sum())
        b = np.bincount(np.minimum((phi[half] + math.pi) / (2 * math.pi) * 16, 15).astype(int), minlength=16)
        assert float(((b - m / 16) ** 2 / (m / 16)).sum()) < 44.3


def test_malleys_sampler_is_cosine_distributed(draws):
    """z = sqrt(1 - s): E z = 2/3 (variance 1/18), E z^2 = 1/2 (variance 1/12), and the world vector has unit length and the
    frame's cosine"""
    n = len(draws["s"])
    z = np.sqrt(1.0 - draws["s"])
    assert abs(z.mean() - 2 / 3) <= 5 * math.sqrt(1 / 18 / n) and abs((z * z).mean() - 0.5) <= 5 * math.sqrt(1 / 12 / n), (z.mean(), (z * z).mean())
    m = 4096
    nrm = sr.unit32(np.random.default_rng(1).normal(size=(m, 3)))
    nrm[0], nrm[1], nrm[2] = (0, 0, 1), (0, 0, -1), (1, 0, 0)               # (the frame's two signs)
    u = {k: a[:m] for k, a in draws.items()}
    d = si.direction(nrm, np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32), np.zeros(m, np.float32), np.zeros(m, np.float32), u, True)
    assert not d["lobe"].any() and not d["no_dir"].any()
    assert np.abs(np.linalg.norm(d["w"], axis=1) - 1).max() < 1e-6 and np.abs(d["cos"] - z[:m]).max() < 1e-6
    t1, t2 = si.frame(nrm.astype(np.float64))
    for a, b in ((t1, t2), (t1, nrm), (t2, nrm)):
        assert np.abs((a * b).sum(1)).max() < 1e-6
    assert np.abs(np.cross(t1, t2) - nrm).max() < 1e-6                      # right-handed


@pytest.mark.parametrize("kappa", [2.0, 50.0, 800.0])
@pytest.mark.parametrize("tilt", [0.0, 0.6, 1.3])
def test_the_density_integrates_to_one(kappa, tilt):
    """by quadrature over the whole sphere of directions around the mirror direction: the lobe technique's density integrates to
    the share of half vectors with wo . h > 0 (1 for wo = n: the integral is 1 there), the cosine technique's to 1 over the
    hemisphere, and so p to q_s share + (1 - q_s).  TOL is the grid's own error: the horizon of the half vectors is an edge inside
    the integrand, across which the midpoint rule converges only like the azimuth's step (at tilt 1.3, kappa 50 the sum is
    0.9650, 0.9680, 0.9695 for 256, 512, 1024 azimuths against a share of 0.9709)"""
    TOL = 8e-3
    n = np.array([[0.0, 0.0, 1.0]])
    wo = np.array([[math.sin(tilt), 0.0, math.cos(tilt)]])
    rough = math.sqrt(2.0 / kappa)
    r = 2.0 * wo[0, 2] * n[0] - wo[0]                                       # the mirror direction
    e1 = np.cross(r, [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(r, e1)
    nt, nph = 3000, 512
    t = (np.arange(nt) + 0.5) / nt
    theta, dth = math.pi * t ** 3, math.pi * 3 * t ** 2 / nt                # fine near the mirror direction
    ph = (np.arange(nph) + 0.5) * (2 * math.pi / nph)
    st, ct = np.sin(theta)[:, None], np.cos(theta)[:, None]
    w = (ct[..., None] * r + (st * np.cos(ph))[..., None] * e1 + (st * np.sin(ph))[..., None] * e2).reshape(-1, 3)
    dw = np.repeat(np.sin(theta) * dth * (2 * math.pi / nph), nph)
    kap = np.full(len(w), float(si.kappa_of(np.float32(rough))))
    Ps, cos, _ = si.density2pi(np.repeat(n, len(w), 0), np.repeat(wo, len(w), 0), w, np.ones(len(w)), kap)
    # (a half vector under the horizon is never drawn; the density clamps n . h' at 0 instead of vanishing there, which no
    # direction above the horizon can reach while wo is above it: n . (w + wo) > 0)
    Ps = np.where(w[:, 2] + wo[0, 2] > 0, Ps, 0.0)
    total_s = float((Ps / (2 * math.pi) * dw).sum())
    total_c = float((np.maximum(cos, 0) / math.pi * dw).sum())
    # the share of the lobe's half vectors with wo . h > 0, by its own quadrature over the hemisphere of n
    k = float(kap[0])
    # (nodes of equal probability: cos(theta) at the CDF's values (i + 1/2) / 4000, 512 azimuths)
    c = 1.0 + np.log((np.arange(4000) + 0.5) / 4000 * (1 - math.exp(-k)) + math.exp(-k)) / k
    hp = (np.arange(512) + 0.5) * (2 * math.pi / 512)
    oh = np.sqrt(1 - c * c)[:, None] * np.cos(hp)[None, :] * wo[0, 0] + c[:, None] * wo[0, 2]
    share = float((oh > 0).mean())
    print(f"kappa {k:.1f} tilt {tilt}: lobe {total_s:.5f} (share {share:.5f}), cosine {total_c:.5f}")
    assert abs(total_c - 1) < 2e-3 and abs(total_s - share) < TOL
    if tilt == 0.0:
        assert share == 1.0 and abs(total_s - 1) < TOL
    for qs in (0.125, 0.5, 0.875):
        P, _, _ = si.density2pi(np.repeat(n, len(w), 0), np.repeat(wo, len(w), 0), w, np.full(len(w), qs), kap)
        up = cos > 0
        both = float((P[up] / (2 * math.pi) * dw[up]).sum()) + qs * float((Ps[~up] / (2 * math.pi) * dw[~up]).sum())
        assert abs(both - (qs * share + (1 - qs))) < TOL, (qs, both)


def test_a_constant_sky_gives_pi_L_with_no_variance():
    """mode 1 with nothing in the way: every path carries pi L exactly"""
    L = (21.0, 32.5, 40.0)
    c = si.constant_case(0, 3, 200, L)
    e = si.emulate(c)
    want = math.pi * np.array(L, np.float32).astype(np.float64)
    assert (e["n_open"] == 200).all() and (e["end"] == 1).all()
    assert (e["terms"][:, :, 0] == want).all() and (e["terms"][:, :, 1] == 0).all()
    assert np.abs(e["out"][:, 0].astype(np.float64) - want).max() <= 2.0 ** -24 * want.max() * 2
    si.check(c, e["out"], e["n_open"], e["trace"], e["end"], emu=e)


# ----------------------------------------------------------------------------------------------------------------------
# the estimator: the uniform sampler's mean, a smaller variance


COPIES = 8192                                                               # 8 points x 8192 = 2^16 paths
# the per-path sample variance of env_dir + env_indir, summed over the points and channels, uniform / brdf, as
# test_the_variance_is_below_the_uniform_samplers prints it (-s)
VARIANCE_RATIOS = {}


@pytest.fixture(scope="module")
def room_paths():
    """the per-path values [paths, 3, 3] of the room with its two sources, two segments: section Y's over 2^16 paths, and over 2^14
    paths each (the brute-force casts are the cost; sigma^ of a difference knows both counts) surfpath_ref's uniform estimator
    and section Y's with the roulette from segment 1 on"""
    cb = si.room_stat_case("plain", COPIES, D=2, S=2, seed=3)
    m = len(cb["pts"]) // 4                                                 # (the same points, materials and counters: the first quarter)
    cu = dict(cb, pts=cb["pts"][:m], nrm=cb["nrm"][:m], face_nrm=cb["face_nrm"][:m], mat={k: a[:m] for k, a in cb["mat"].items()})
    out = {"uniform": sp.emulate(cu)["out"].astype(np.float64)}
    for name, c in (("brdf", cb), ("roulette", dict(cu, rr=1))):
        e = si.emulate(c)
        out[name] = e["out"].astype(np.float64)
        out[name + " ends"] = np.bincount(e["end"].ravel(), minlength=5)
        out[name + " cast"] = e["cast"].mean()
    return out


def _same_mean(a, b, what):
    diff = a.mean(0) - b.mean(0)
    sigma = np.sqrt(a.var(0, ddof=1) / len(a) + b.var(0, ddof=1) / len(b))
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.where(sigma > 0, np.abs(diff) / sigma, np.where(diff == 0, 0.0, np.inf))
    print(f"{what}: |difference of the means| / sigma^ per component and channel\n{np.round(z, 2)}\nmeans {a.mean(0).ravel().round(5)} / {b.mean(0).ravel().round(5)}")
    assert (z <= 4.0).all(), (what, z)
    assert (a.mean(0) > 0).all() and (b.mean(0) > 0).all()


def test_the_mean_is_the_uniform_samplers(room_paths):
    assert len(room_paths["brdf"]) >= 1 << 16
    _same_mean(room_paths["brdf"], room_paths["uniform"], "brdf against uniform")


def test_the_roulette_keeps_the_mean(room_paths):
    _same_mean(room_paths["roulette"], room_paths["brdf"], "roulette from segment 1 against none")
    _same_mean(room_paths["roulette"], room_paths["uniform"], "roulette from segment 1 against uniform")
    ends = room_paths["roulette ends"]
    print(f"ends {ends.tolist()} (none: {room_paths['brdf ends'].tolist()}); rays a path: {room_paths['roulette cast']:.2f} (none: {room_paths['brdf cast']:.2f})")
    assert ends[3] > 500 and room_paths["brdf ends"][3] == 0 and room_paths["roulette cast"] < room_paths["brdf cast"]


@pytest.mark.parametrize("kind", ["diffuse", "glossy"])
def test_the_variance_is_below_the_uniform_samplers(kind):
    """the room all diffuse (roughness 1, metallic 0), and a glossy copy (roughness 0.1, metallic 1): the per-path sample
    variance of env_dir + env_indir per point and channel, summed over both -- the variance of the image.  (Per point the
    ratio is printed, not asserted: at a point that sees the sky through one bounce in a thousand, 2 048 paths do not estimate a
    variance.)"""
    copies = 2048
    c = si.room_stat_case(kind, copies, D=3, S=0, seed=11)
    both = {}
    for name, fn in (("uniform", sp.emulate), ("brdf", si.emulate)):
        o = fn(c)["out"].astype(np.float64)
        both[name] = (o[:, 0] + o[:, 1]).reshape(copies, 8, 3)
    var = {k: x.var(0, ddof=1) for k, x in both.items()}                    # [8 points, 3 channels]
    ratio = float(var["uniform"].sum() / var["brdf"].sum())
    lit = var["uniform"].sum(1) > 0
    print(f"{kind}: variance uniform / brdf = {ratio:.2f} (summed over {int(lit.sum())} lit points and 3 channels); per lit point "
          f"{(var['uniform'].sum(1)[lit] / np.maximum(var['brdf'].sum(1)[lit], 1e-300)).round(2).tolist()}; means "
          f"{both['uniform'].mean((0, 1)).round(4).tolist()} / {both['brdf'].mean((0, 1)).round(4).tolist()}")
    assert lit.sum() >= 3 and var["brdf"].sum() < var["uniform"].sum()


# ----------------------------------------------------------------------------------------------------------------------
# the emulation inside the GPU's checks, its mutants outside


def test_emulation_passes_every_gpu_check_with_no_ambiguous_decision():
    worst = {k: 0.0 for k in si.K_FAMILY}
    ends = np.zeros(5, np.int64)
    lobes = [0, 0]
    for name, c in si.generic_cases().items():
        e = si.emulate(c)
        w, amb = si.check(c, e["out"], e["n_open"], e["trace"], e["end"], emu=e, what=name)
        assert amb == 0, (name, amb)
        for fam, x in w.items():
            worst[fam] = max(worst[fam], x)
        ends += np.bincount(e["end"].ravel(), minlength=5)
        for seg in e["segs"]:
            lobes[0] += int(seg["lobe"].sum())
            lobes[1] += int((~seg["lobe"]).sum())
        print(f"{name:28s} worst ratio {w}, ends {np.bincount(e['end'].ravel(), minlength=5).tolist()}")
    print("worst ratios of the emulation:", worst, "of", si.K_FAMILY, "ends", ends.tolist(), "lobe / cosine draws", lobes)
    assert (ends > 100).all(), "the cases see every end code"
    assert min(lobes) > 1000
    c = si.zero_rough_case()
    e = si.emulate(c)
    assert si.check(c, e["out"], e["n_open"], e["trace"], e["end"], emu=e, values=False)[1] == 0 and np.isfinite(e["out"]).all()
    assert e["out"].max() > 0


VALUE_MUTANTS = ("no_4oh", "p_without_qs", "norm_2kappa", "no_mis", "T_not_divided", "mode1_2pi_cos")


@pytest.mark.parametrize("mutant", si.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    c = si.mutant_case(mutant)
    e = si.emulate(c)
    si.check(c, e["out"], e["n_open"], e["trace"], e["end"], emu=e, what="the emulation itself")
    m = si.emulate(c, mutant)
    with pytest.raises(AssertionError):
        si.check(c, m["out"], m["n_open"], m["trace"], m["end"], emu=e, what=mutant)
    if mutant in VALUE_MUTANTS:
        # a wrong weight shows in the values alone, whatever it does to the roulette's decisions
        with pytest.raises(AssertionError, match="the bound does not hold"):
            si.check(c, m["out"], emu=e, what=mutant)


def test_the_required_mutants_are_listed():
    assert set(si.MUTANTS) == {"no_4oh", "p_without_qs", "kappa_from_ro", "norm_2kappa", "no_mis", "T_not_divided", "rr_late", "frame_swapped",
                               "cos_z_linear", "purpose_2b", "word_reused", "mode1_2pi_cos"}
    assert set(si.K_FAMILY) == set(sp.K_FAMILY) and si.MIN_ROUGH == 0.05 and si.AMBIGUOUS_CAP == 0.001
