"""Environment light on the surface without a GPU: the product's direction table, the restatement's flip and environment
against what the reference computes (tests/golden/surfenv.npz, written by tools/gen_surfenv_golden.py), closed forms, the
binary-structure emulation (tests/surfenv_ref.py) inside every check the GPU has to pass with no ambiguous direction in the
generic cases, its mutants outside, the header's entry against the binding, and the input errors of the Python layer (raised
before anything is launched)."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import surfenv_ref as sv
from conftest import ROOT, load_npz

U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    return load_npz("surfenv.npz")


@pytest.fixture(scope="module")
def generic():
    return {name: (c, sv.emulate(c)) for name, c in sv.generic_cases().items()}


@pytest.mark.parametrize("n", [1, 2, 16, 17, 128, 256])
def test_hemisphere_directions_are_the_references_bits(golden, n):
    from esr_nerf_amd import sources
    got = sources.hemisphere_directions(n)
    want = golden[f"table_{n}"]
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 3)
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    # the restatement's own table (float64, rounded once) is the same table to a binary32 rounding of the angle
    assert np.abs(sv.table(n).astype(np.float64) - want).max() <= 2e-4
    assert (want[:, 2] > 0).all() and abs(want[:, 2].astype(np.float64).mean() - 0.5) <= U24


def test_hemisphere_directions_refuse_bad_counts():
    from esr_nerf_amd import sources
    for n in (0, -3, sv.MAX_DIRS + 1):
        with pytest.raises(ValueError):
            sources.hemisphere_directions(n)


def test_the_flip_is_the_references(golden):
    n, want = golden["flip_normals"], golden["flip_dirs"]
    w, s = sv.flip(golden["table_16"], n)
    assert np.array_equal(w.view(np.uint32), want.view(np.uint32))
    assert (s[0] > 0).all() and (s[1] < 0).all() and (s[3] < 0).any() and (s[3] > 0).any()


def test_the_environment_is_the_references(golden):
    """float64 restatement, the binary32 emulation and the repository's SphericalGaussian against the reference's binary32
    output: within the reference's own rounding -- 48 products and additions, an exponential and the softplus, each 2^-24 of
    the sum of magnitudes, which `absref` of the error algebra states"""
    from esr_nerf_amd.esrnerf import SphericalGaussian
    sg = (golden["sg_mus"], golden["sg_lambdas"], golden["sg_lobes"])
    d, want = golden["sg_dirs"], golden["sg_out"].astype(np.float64)
    value, E = sv.env_ref(sg, d)
    absref = E + np.abs(value)                                            # (the algebra's E and the reference's own last rounding)
    e64 = sv.env64(sg, d)
    assert (np.abs(e64 - want) <= U24 * absref).all(), float((np.abs(e64 - want) / (U24 * absref)).max())
    e32 = sv.env32(sg, d).astype(np.float64)
    assert (np.abs(e32 - e64) <= U24 * absref).all()
    own = SphericalGaussian(48)
    with torch.no_grad():
        for k, x in zip(("mus", "lambdas", "lobes"), sg):
            getattr(own, k).copy_(torch.from_numpy(x))
        got = own(torch.from_numpy(d)).numpy().astype(np.float64)
    assert (np.abs(got - e64) <= U24 * absref).all()
    print("worst |restatement - reference| / (2^-24 absref):", float((np.abs(e64 - want) / (U24 * absref)).max()))


@pytest.mark.parametrize("R", [16, 128, 256])
def test_a_constant_environment_gives_pi_L(golden, R):
    """one lobe at lambda = 0, normal +z, no mesh: the irradiance of a constant radiance L is pi L; the table's cos has the
    mean 1/2 exactly, up to the binary32 rounding of each entry"""
    L = (21.0, 32.5, 40.0)
    c = sv.make_case(sv.no_face(), golden[f"table_{R}"], sv.sg_constant(L), [[0.1, 0.2, 0.3]], [[0.0, 0.0, 1.0]], 1, bitexact=True)
    e = sv.emulate(c)
    assert e["n_open"][0] == R and (e["hit"] == 0).all()
    want = math.pi * np.array(L)
    assert (np.abs(e["out"][0].astype(np.float64) - want) <= 2 * U24 * want).all(), (e["out"][0], want)
    sv.check(c, e["out"], e["n_open"], e["hit"], emu=e)


def test_nothing_is_open_under_a_slab(generic):
    for mode in (0, 1):
        c = sv.slab_case(mode)
        e = sv.emulate(c)
        assert e["n_open"][0] == 0 and (e["hit"] == 1).all() and (e["out"] == 0).all() and not e["ambiguous"].any()


def test_emulation_passes_every_gpu_check_with_no_ambiguous_direction(generic):
    worst = {k: 0.0 for k in sv.K_FAMILY}
    for name, (c, e) in generic.items():
        w, amb = sv.check(c, e["out"], e["n_open"], e["hit"], emu=e, what=name)
        assert amb == 0, (name, amb, np.argwhere(e["ambiguous"])[:4].tolist())
        worst[sv.family(c)] = max(worst[sv.family(c)], w)
        print(f"{name:40s} worst ratio {w:.3f}, open {int(e['n_open'].sum())} of {e['hit'].size}")
    print("worst ratios of the emulation:", worst, "of", sv.K_FAMILY)
    for fam, w in worst.items():
        assert w <= sv.K_FAMILY[fam]
    both = [e["hit"] for name, (c, e) in generic.items() if name.startswith("R=")]
    assert all((h == 0).any() and (h == 1).any() for h in both), "the generic cases see hits and misses"


def test_constructed_ambiguity_sits_where_it_was_built(generic):
    for name, (c, allowed) in sv.constructed_cases().items():
        e = sv.emulate(c)
        assert e["ambiguous"].any() and not (e["ambiguous"] & ~allowed).any(), (name, np.argwhere(e["ambiguous"]).tolist())
        sv.check(c, e["out"], e["n_open"], e["hit"], emu=e, what=name)
    c, e = generic["t_min met exactly"]
    assert e["n_open"][0] == 1, "t == t_min is outside the interval"
    c, e = generic["tie"]
    assert e["out"][0, 0] != sv.emulate(c, "serial_sum")["out"][0, 0]


def _mutant_cases(mutant):
    modes = (1,) if mutant in sv.MODE1_ONLY + ("serial_sum",) else (0, 1)
    for mode in modes:
        if mutant == "serial_sum":
            yield sv.tie_case()                                          # (the planted tie needs exact terms: mode 1)
        elif mutant == "t_min_inclusive":
            yield sv.t_min_case(mode)
        elif mutant == "face_ignored":
            yield sv.own_face_case(mode)
        elif mutant == "flip_by_face_normal":
            yield sv.on_mesh_case(mode, False)
        elif mutant == "divide_by_padded":
            yield sv.shape_case(4, 3, 48, "room", mode, False)
        else:
            yield sv.shape_case(4, 16, 48, "room", mode, mutant in sv.VRAD_ONLY)


@pytest.mark.parametrize("mutant", sv.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    n = 0
    for c in _mutant_cases(mutant):
        e = sv.emulate(c)
        sv.check(c, e["out"], e["n_open"], e["hit"], emu=e, what="the emulation itself")
        m = sv.emulate(c, mutant)
        with pytest.raises(AssertionError):
            sv.check(c, m["out"], m["n_open"], m["hit"], emu=e, what=mutant)
        n += 1
    assert n == (1 if mutant in sv.MODE1_ONLY + ("serial_sum",) else 2)


def test_the_entry_is_the_headers():
    from esr_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    assert _lib.SURFACE_ENV_MAX_DIRS == sv.MAX_DIRS == 4096 and _lib.SURFACE_ENV_MAX_SG == sv.MAX_SG == 64
    assert "esr_surface_env" in _lib.EXPORTS and len(_lib.SIGNATURES["esr_surface_env"][1]) == 26
    assert _lib.ABI_VERSION == int(re.search(r"#define ESR_ABI_VERSION (\d+)", header).group(1)) >= 45
    assert re.search(r"\n \* V\. Environment light on the surface", header)


def _cpu_surface():
    from esr_nerf_amd import sources
    v, tr = sv.room()
    V = len(v)
    attrs = dict(normal=torch.zeros(V, 3), basecolor=torch.zeros(V, 3), roughness=torch.zeros(V), metallic=torch.zeros(V),
                 emission=torch.zeros(V, 3))
    return sources.Surface(torch.from_numpy(v), torch.from_numpy(tr), attrs)


def test_python_layer_refuses_bad_inputs_before_any_launch():
    from esr_nerf_amd import sources
    surf = _cpu_surface()
    P = 5
    pts, nrm = torch.zeros(P, 3, dtype=torch.float64), torch.zeros(P, 3)
    env = tuple(torch.from_numpy(x) for x in sv.sg_random(48, 0))
    V = surf.vertices.shape[0]
    bad = [dict(env=None), dict(env=env[:2]), dict(env=(env[0], env[1][:7], env[2])), dict(env=(env[0].int(), env[1], env[2])),
           dict(env=tuple(torch.from_numpy(x) for x in sv.sg_random(65, 0))), dict(points=pts[:, :2]), dict(points=pts.int()),
           dict(normals=nrm[:4]), dict(dirs=0), dict(dirs=4097), dict(dirs=True), dict(dirs=torch.zeros(4, 2)),
           dict(dirs=torch.zeros(4097, 3)), dict(dirs=16.0), dict(t_min=-1.0), dict(t_min=float("nan")), dict(wo=nrm),
           dict(wo=nrm, basecolor=nrm, roughness=nrm[:, 0], metallic=nrm[:3, 0]), dict(faces=torch.zeros(P, dtype=torch.int64)),
           dict(faces=torch.zeros(P - 1, dtype=torch.int32)), dict(vertex_radiance=torch.zeros(V - 1, 3)), dict(bvh="tree")]
    for kw in bad:
        args = dict(env=env, points=pts, normals=nrm)
        args.update(kw)
        with pytest.raises(ValueError):
            sources.environment_light(surf, **args)


def _stub_raycast(monkeypatch, H, W):
    """lit_view's three calls into the ray caster, answered for a surface without a face: every pixel misses"""
    from esr_nerf_amd import raycast
    N = H * W
    monkeypatch.setattr(raycast, "build", lambda v, t: "bvh")
    monkeypatch.setattr(raycast, "pixel_rays", lambda cams, view: (torch.zeros(N, 3, dtype=torch.float64), torch.ones(N, 3, dtype=torch.float64), None))
    monkeypatch.setattr(raycast, "cast", lambda bvh, o, d: types.SimpleNamespace(
        face=torch.full((N,), -1, dtype=torch.int32), t=torch.full((N,), float("inf"), dtype=torch.float64), bary=torch.zeros(N, 2, dtype=torch.float64)))


def test_lit_view_keeps_its_keys_without_an_environment(monkeypatch):
    from esr_nerf_amd import sources
    H, W = 3, 4
    _stub_raycast(monkeypatch, H, W)
    surf = sources.Surface(torch.zeros(3, 3, dtype=torch.float64), torch.zeros(0, 3, dtype=torch.int64), {"emission": torch.zeros(3, 3)})
    z3, z1 = torch.zeros(0, 3, dtype=torch.float64), torch.zeros(0, dtype=torch.float64)
    rep = sources.SourceReport(0.1, torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int64), z1, z3, z3, z3, z3, z1.float(), z3, z3)
    cams = types.SimpleNamespace(n_views=1, device=torch.device("cpu"), width=W, height=H)
    img = sources.lit_view(surf, rep, cams, 0)
    assert set(img) == {"lin/reflect", "lin/emit", "face", "depth"}
    env = tuple(torch.from_numpy(x) for x in sv.sg_random(48, 0))
    lit = sources.lit_view(surf, rep, cams, 0, env=env, env_dirs=16)
    assert set(lit) == set(img) | {"lin/env_dir", "etc/open"}
    two = sources.lit_view(surf, rep, cams, 0, env=env, env_dirs=16, bounces=1)
    assert set(two) == set(lit) | {"lin/env_indir"}
    for k in img:
        assert torch.equal(img[k], lit[k]) and torch.equal(img[k], two[k]), k
    assert tuple(two["lin/env_dir"].shape) == (H, W, 3) and tuple(two["etc/open"].shape) == (H, W) and float(two["lin/env_indir"].abs().max()) == 0.0
    for kw in (dict(env=env, bounces=2), dict(env=env, bounces=True), dict(env=env, env_dirs=0), dict(env=env[:2])):
        with pytest.raises(ValueError):
            sources.lit_view(surf, rep, cams, 0, **kw)
