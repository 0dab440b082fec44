"""Path-traced light on the surface without a GPU: Philox4x32-10 against its known answers, the direction sampler's moments, closed
forms (a constant environment, the mean of the sources' gather over the slots, one segment against the direction table of
tests/surfenv_ref.py), the binary-structure emulation (tests/surfpath_ref.py) inside every check the GPU has to pass with no
ambiguous decision in the generic cases, its mutants outside, the header's entry against the binding, and the input errors of the
Python layer (raised before anything is launched)."""
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
import surfpath_ref as sp
from conftest import ROOT


@pytest.fixture(scope="module")
def generic():
    return {name: (c, sp.emulate(c)) for name, c in sp.generic_cases().items()}


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = sp.philox(*counter, key)
    assert got.dtype == np.uint32 and " ".join(f"{int(x):08x}" for x in got) == want
    # on arrays, and the seed's two words are the key
    many = sp.philox(np.full(5, counter[0]), counter[1], np.full((3, 1), counter[2]), counter[3], key)
    assert many.shape == (3, 5, 4) and (many == got).all()
    assert sp.seed_key(key[0] | key[1] << 32) == key


def test_the_sampler_is_uniform_on_the_sphere():
    """2^20 directions at a fixed seed, flipped into the hemisphere of a normal: uniform there, E cos = 1/2 (variance 1/12) and
    E cos^2 = 1/3 (variance 1/5 - 1/9 = 4/45); the azimuth of the unflipped direction uniform over 16 bins (chi^2, 15 degrees of
    freedom: 44.3 is the 1e-4 quantile); unit length to a few roundings"""
    n = 1 << 20
    w, fallback = sp.sphere(np.arange(n), 7, 2, sp.seed_key(0xC0FFEE1234))
    assert w.shape == (n, 3) and not fallback.any()
    assert np.abs(np.sqrt((w * w).sum(1)) - 1.0).max() <= 2.0 ** -50
    nrm = sr.unit32(np.array([[0.3, -0.5, 0.8]]))
    fl, s = sv.flip(w.astype(np.float32), nrm)
    cos = sr._dot(nrm.astype(np.float64), fl[0].astype(np.float64))
    assert (cos >= -1e-7).all()
    assert abs(cos.mean() - 0.5) <= 5 * math.sqrt(1 / 12 / n), cos.mean()
    assert abs((cos * cos).mean() - 1 / 3) <= 5 * math.sqrt(4 / 45 / n), (cos * cos).mean()
    bins = np.bincount(np.minimum((np.arctan2(w[:, 1], w[:, 0]) + math.pi) / (2 * math.pi) * 16, 15).astype(int), minlength=16)
    chi2 = float(((bins - n / 16) ** 2 / (n / 16)).sum())
    assert chi2 < 44.3, chi2
    print(f"E cos {cos.mean():.5f}, E cos^2 {(cos * cos).mean():.5f}, chi^2 {chi2:.1f}, flipped {float((s < 0).mean()):.4f}")


def test_the_sampler_takes_the_first_pair_inside_the_disc():
    top, half = 0xFFFFFFFF, 0x80000000                                     # a = 1 - 2^-31 and a = 0
    out = np.full((8, 4), top, np.uint32)                                   # every pair outside: s = 2 (1 - 2^-31)^2 > 1
    w, fb = sp.sphere_from_words(out)
    assert fb and np.array_equal(w, [0.0, 0.0, 1.0]), "the fallback"
    words = out.copy()
    words[7, 2:] = (half, half)                                             # the sixteenth candidate, the centre: s = 0
    w, fb = sp.sphere_from_words(words)
    assert not fb and np.array_equal(w, [0.0, 0.0, 1.0])
    words[3, :2] = (half, 0xC0000000)                                       # an earlier one wins: a = (0, 1/2), s = 1/4
    w, fb = sp.sphere_from_words(words)
    assert not fb and np.array_equal(w, [0.0, 2.0 * 0.5 * math.sqrt(0.75), 0.5])
    words[3, :2] = (0, half)                                                # a = (-1, 0): s = 1 is outside
    assert np.array_equal(sp.sphere_from_words(words)[0], [0.0, 0.0, 1.0])
    # the lazy draw of `sphere` is the draw of all eight blocks
    key = sp.seed_key(5)
    c0 = np.arange(4096)
    full = np.stack([sp.philox(c0, 1, 4, blk, key) for blk in range(8)], -2)
    assert np.array_equal(sp.sphere(c0, 1, 4, key)[0], sp.sphere_from_words(full)[0])
    share = (((2.0 * (full[:, 0, :2].astype(np.float64) * 2.0 ** -32) - 1.0) ** 2).sum(1) < 1).mean()
    assert abs(share - math.pi / 4) < 0.03


def test_a_constant_environment_gives_pi_L():
    """mode 1 under a constant radiance L without a face: pi L, to the noise of N = 4096 uniform directions (the variance of cos
    on the hemisphere is 1/12: sigma = 2 pi L / sqrt(12 N) = pi L / sqrt(3 N))"""
    L, N = (21.0, 32.5, 40.0), 4096
    c = sp.make_case(0, 2, N, 1, 0, 1, 1, 1, sg=sv.sg_constant(L), nrm=[[0.0, 0.0, 1.0], [0.6, 0.0, -0.8]], pts=[[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]], bitexact=True)
    e = sp.emulate(c)
    want = math.pi * np.array(L)
    assert (e["n_open"] == N).all() and (e["end"] == 1).all() and (e["trace"] == -1).all()
    assert (np.abs(e["out"][:, 0].astype(np.float64) - want) <= 5 * want / math.sqrt(3 * N)).all(), (e["out"][:, 0], want)
    assert (e["out"][:, 1:] == 0).all()
    sp.check(c, e["out"], e["n_open"], e["trace"], e["end"], emu=e)


def test_the_gather_averages_to_the_direct_light():
    """The sources' term with the slot forced to k, averaged over all Kp slots, is the direct light of surflight_ref at the vertex
    the segment reached: Kp term_k / Kp summed over k is section U's sum over the slots"""
    c = sp.make_case("room", 6, 2, 1, 2, 16, 48, 1, seed=5)
    kp = c["L"]["weight"].shape[1]
    runs = [sp.emulate(dict(c, force_slot=k)) for k in range(kp)]
    seg = runs[0]["segs"][0]
    go, vx = seg["go"], seg["vertex"]
    assert len(go) >= 4
    mean = np.mean([r["out"][:, 2].astype(np.float64) for r in runs], 0)              # [P, 3]
    direct = sr.emulate(dict(v=c["v"], tr=c["tr"], L=c["L"], pts=vx["x"], nrm=vx["n"], mode=0, eps=c["eps"], face_nrm=vx["n"],
                             mat=dict(base=vx["base"], rough=vx["rough"], metal=vx["metal"], wo=vx["wo"])))["sum64"].sum(1)
    want = np.zeros((len(c["pts"]) * c["N"], 3))
    want[go] = seg["T"] * direct
    want = want.reshape(len(c["pts"]), c["N"], 3).sum(1) / c["N"]
    assert want.max() > 0 and np.abs(mean - want).max() <= 1e-6 * want.max(), (mean, want)


# |path tracer - table| per point and channel in units of sigma^ = std(the N per-path terms) / sqrt(N), and the table's own error
# |R = 2048 - R = 4096| beside it, as test_one_segment_is_the_environment_light measured them (-s prints them): the worst
# |difference| is 0.93 sigma^ over the values of the three points that see the sky; the table's own error is up to 5.97e-3
# (0.27 sigma^ there)
ONE_SEGMENT_MEASURED = dict(worst_sigmas=0.93, table_error=5.97e-3)


def test_one_segment_is_the_environment_light():
    """mode 0, D = 1, no source, on the room's points: env_dir is the Monte-Carlo estimate of what surfenv_ref's reference
    integrates with the table of R = 4096 directions.  Within 6 sigma^ of it plus the table's own error, measured as the
    difference between R = 2048 and R = 4096"""
    v, tr = sp.scene("room")[0][:2]
    pts = rr.room_points()
    nrm = sr.unit32(np.tile([[0.1, -0.2, 1.0]], (len(pts), 1)))
    N = 4096
    c = sp.make_case("room", len(pts), N, 1, 0, 1, 48, 0, seed=3, pts=pts, nrm=nrm, t_min=1e-6)
    e = sp.emulate(c)
    got = e["out"][:, 0].astype(np.float64)
    sigma = e["terms"][:, :, 0].std(1, ddof=1) / math.sqrt(N)
    ref = {}
    for R in (2048, 4096):
        ce = sv.make_case((v, tr), R, c["sg"], pts, nrm, 0, t_min=1e-6)
        ce["mat"] = c["mat"]
        ref[R] = sv.reference(ce, sv.emulate(ce))[0]
    table = np.abs(ref[2048] - ref[4096])
    diff = np.abs(got - ref[4096])
    seen = sigma > 0
    print(f"worst |path - table| / sigma^ {float((diff[seen] / sigma[seen]).max()):.2f}; the table's own error up to {table.max():.2e} "
          f"({float((table[seen] / sigma[seen]).max()):.2f} sigma^); open {e['n_open'].tolist()} of {N}")
    assert (diff <= 6 * sigma + table).all(), (diff, sigma, table)
    assert (got[e["n_open"] == 0] == 0).all() and seen.any()


def test_emulation_passes_every_gpu_check_with_no_ambiguous_decision(generic):
    worst = {k: 0.0 for k in sp.K_FAMILY}
    for name, (c, e) in generic.items():
        w, amb = sp.check(c, e["out"], e["n_open"], e["trace"], e["end"], emu=e, what=name)
        assert amb <= sp.AMBIGUOUS_CAP * e["ambiguous"].size, (name, amb)
        if c["scene"] in ("room", "window"):
            assert amb == 0, (name, amb, np.argwhere(e["ambiguous"])[:4].tolist())
        for fam, x in w.items():
            worst[fam] = max(worst[fam], x)
        print(f"{name:28s} worst ratio {w}, ends {np.bincount(e['end'].ravel(), minlength=3).tolist()}")
    print("worst ratios of the emulation:", worst, "of", sp.K_FAMILY)
    ends = np.concatenate([e["end"].ravel() for _, e in generic.values()])
    assert all((ends == k).sum() > 100 for k in range(3)), "the cases see paths that use up the depth, leave the mesh and reach a back face"
    c, e = generic["tie"]
    assert e["out"][0, 0, 1] != sp.emulate(c, "serial_sum")["out"][0, 0, 1]


@pytest.mark.parametrize("mutant", sp.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    for fam in sp.MUTANT_FAMILIES[mutant]:
        c = sp.mutant_case(mutant, fam)
        e = sp.emulate(c)
        sp.check(c, e["out"], e["n_open"], e["trace"], e["end"], emu=e, what="the emulation itself")
        m = sp.emulate(c, mutant)
        with pytest.raises(AssertionError):
            sp.check(c, m["out"], m["n_open"], m["trace"], m["end"], emu=e, what=mutant, families=(fam,))


def test_the_required_mutants_are_listed():
    assert set(sp.MUTANTS) >= {"no_flip", "flip_by_face_normal", "skip_not_updated", "wo_not_negated", "throughput_not_carried",
                               "first_material_at_bounces", "nee_without_kp", "nee_at_first_vertex", "emission_on_source_hit",
                               "miss0_in_indir", "divide_by_padded", "counter_without_b", "counter_without_point_base", "serial_sum",
                               "mode1_weight_every_segment"}
    assert set(sp.MUTANT_FAMILIES) == set(sp.MUTANTS) and all(set(f) <= set(sp.K_FAMILY) and f for f in sp.MUTANT_FAMILIES.values())


def test_the_entry_is_the_headers():
    import ctypes as C
    from esr_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    assert _lib.SURFACE_PATH_MAX_PATHS == sp.MAX_PATHS == 4096 and _lib.SURFACE_PATH_MAX_DEPTH == sp.MAX_DEPTH == 8
    proto = re.search(r"\nint esr_surface_path\(([^)]*)\);", header).group(1)
    params = [" ".join(p.split()) for p in proto.split(",")]
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    want = [C.c_void_p if "*" in p else kinds[p.rsplit(" ", 1)[0]] for p in params]
    assert len(params) == 40 and _lib.SIGNATURES["esr_surface_path"] == (C.c_int, want) and "esr_surface_path" in _lib.EXPORTS
    names = [p.replace("*", " ").split()[-1] for p in params]
    assert names[:5] == ["nodes", "n_faces", "vertices", "n_vertices", "triangles"] and names[-5:] == ["out", "n_open", "trace", "end", "stream"]
    assert [names[i] for i, p in enumerate(params) if "*" not in p] == ["n_faces", "n_vertices", "n_sources", "slots", "eps", "n_sg", "n_points",
                                                                       "mode", "n_paths", "depth", "t_min", "seed", "point_base"]
    assert _lib.ABI_VERSION == int(re.search(r"#define ESR_ABI_VERSION (\d+)", header).group(1)) >= 47
    assert re.search(r"\n \* X\. Path-traced light on the surface", header)


def _cpu_surface():
    from esr_nerf_amd import sources
    v, tr, fs, S = rr.room()
    V = len(v)
    attrs = dict(normal=torch.zeros(V, 3), basecolor=torch.zeros(V, 3), roughness=torch.zeros(V), metallic=torch.zeros(V),
                 emission=torch.zeros(V, 3))
    z3, z1 = torch.zeros(0, 3, dtype=torch.float64), torch.zeros(0, dtype=torch.float64)
    rep = sources.SourceReport(0.1, torch.zeros(len(tr), dtype=torch.int32) - 1, torch.zeros(0, dtype=torch.int64), z1, z3, z3, z3, z3, z1.float(), z3, z3)
    return sources.Surface(torch.from_numpy(v), torch.from_numpy(tr), attrs), rep


def test_python_layer_refuses_bad_inputs_before_any_launch():
    from esr_nerf_amd import sources
    surf, rep = _cpu_surface()
    P = 5
    pts, nrm = torch.zeros(P, 3, dtype=torch.float64), torch.zeros(P, 3)
    env = tuple(torch.from_numpy(x) for x in sv.sg_random(48, 0))
    mat = dict(basecolor=nrm, roughness=nrm[:, 0], metallic=nrm[:, 0], wo=nrm)
    bad = [dict(paths=0), dict(paths=4097), dict(paths=True), dict(paths=4.0), dict(depth=0), dict(depth=9), dict(mode=2), dict(seed=-1),
           dict(seed=2 ** 64), dict(seed=1.5), dict(chunk=0), dict(samples=0), dict(samples=65), dict(t_min=-1.0), dict(t_min=float("nan")),
           dict(eps=0.5), dict(env=env[:2]), dict(env=tuple(torch.from_numpy(x) for x in sv.sg_random(65, 0))), dict(points=pts[:, :2]),
           dict(points=pts.int()), dict(normals=nrm[:4]), dict(faces=torch.zeros(P, dtype=torch.int64)), dict(faces=torch.zeros(P - 1, dtype=torch.int32)),
           dict(wo=None), dict(metallic=nrm[:3, 0]), dict(bvh="tree")]
    for kw in bad:
        args = dict(points=pts, normals=nrm, env=env, **mat)
        args.update(kw)
        with pytest.raises(ValueError):
            sources.path_light(surf, rep, **args)
    bare = sources.Surface(surf.vertices, surf.triangles, {"emission": torch.zeros(surf.vertices.shape[0], 3)})
    with pytest.raises(ValueError):
        sources.path_light(bare, rep, pts, nrm, env=env, bvh=None, **mat)


def test_lit_view_takes_paths_and_keeps_its_keys_without(monkeypatch):
    """a surface without a face (every pixel misses: nothing is launched): the keys with and without paths, and the refusals"""
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
    cams = types.SimpleNamespace(n_views=1, device=torch.device("cpu"), width=W, height=H)
    env = tuple(torch.from_numpy(x) for x in sv.sg_random(48, 0))
    plain = sources.lit_view(surf, rep, cams, 0)
    assert set(plain) == {"lin/reflect", "lin/emit", "face", "depth"}
    assert set(sources.lit_view(surf, rep, cams, 0, env=env, env_dirs=16, bounces=1)) == set(plain) | {"lin/env_dir", "etc/open", "lin/env_indir"}
    for kw in (dict(env=env), dict()):
        traced = sources.lit_view(surf, rep, cams, 0, paths=4, depth=2, seed=3, **kw)
        assert set(traced) == set(plain) | {"lin/env_dir", "lin/env_indir", "lin/src_indir", "etc/open"}
        for k in plain:
            assert torch.equal(plain[k], traced[k]), k
        assert tuple(traced["lin/src_indir"].shape) == (H, W, 3) and tuple(traced["etc/open"].shape) == (H, W)
    for kw in (dict(paths=4, bounces=1), dict(paths=0), dict(paths=4097), dict(paths=4, depth=9), dict(paths=4, depth=0), dict(paths=4, seed=-1),
               dict(paths=True), dict(paths=4, env=env[:2])):
        with pytest.raises(ValueError):
            sources.lit_view(surf, rep, cams, 0, **kw)
