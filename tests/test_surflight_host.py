"""Surface lighting without a GPU: the restatement (tests/surflight_ref.py) against the closed form of a square emitter, the
binary-structure emulation inside every check the GPU has to pass, its mutants outside, the light arrays of
sources.source_lights against a direct numpy loop, the argument struct against the header, and the input errors of the
Python layer (raised before anything is launched)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import raycast_ref as rr
import surflight_ref as sr
from conftest import ROOT


@pytest.fixture(scope="module")
def cases():
    out = {}
    for mode in (1, 0):
        for name, c in sr.room_cases(mode).items():
            out[f"mode {mode} {name}"] = (c, sr.emulate(c))
    return out


@pytest.mark.parametrize("h, bound", [(3, 1e-3), (10, 1e-3)])
def test_irradiance_of_a_square_matches_the_closed_form(h, bound):
    """128 faces, 64 samples, on the axis at h sides: 3.6e-4 off at h = 3 and 3.4e-5 at h = 10"""
    c = sr.square_case(h)
    got = float(sr.emulate(c)["sum64"][0, 0, 0])
    want = sr.closed_form_square(1.0, h)
    print(f"h = {h}: estimator {got:.9g}, closed form {want:.9g}, relative {abs(got - want) / want:.3g}")
    assert int(c["L"]["n"][0]) == 64 and abs(got - want) <= bound * want


def test_the_estimator_is_low_in_the_near_field():
    """at 0.05 sides, well inside one sample spacing (1/8 side), the clamp max(r2, A) holds the estimate under the closed
    form: the documented limit"""
    c = sr.square_case(0.05)
    got, want = float(sr.emulate(c)["sum64"][0, 0, 0]), sr.closed_form_square(1.0, 0.05)
    print(f"h = 0.05: estimator {got:.6g}, closed form {want:.6g}")
    assert 0.0 < got < 0.6 * want


def test_emulation_passes_every_gpu_check_with_no_ambiguous_segment(cases):
    worst = {0: 0.0, 1: 0.0}
    for name, (c, e) in cases.items():
        w, amb = sr.check(c, e["out"], e["seen"], emu=e, what=name)
        assert amb == 0, (name, amb)
        assert (e["seen"] == 1).sum() >= 6 and (e["seen"] == 2).sum() >= 1, (name, np.bincount(e["seen"].ravel()))
        worst[c["mode"]] = max(worst[c["mode"]], w)
        print(f"{name:40s} worst ratio {w:.3f}")
    print("worst: mode 1", worst[1], "of K_IRR", sr.K_IRR, "; mode 0", worst[0], "of", sr.K_FAMILY["reflect"])


def test_special_points_are_silent(cases):
    c, e = cases["mode 1 room/16 special"]
    seen = e["seen"]
    assert (seen[0, 0] == 0).all() and (seen[1, 0] == 0).all()           # coplanar with source 0: cos_l is exactly 0
    assert seen[2, 0, 0] == 0                                            # at the sample: r2 = 0
    assert (seen[3] == 0).all() and (e["out"][3] == 0).all()             # a NaN coordinate
    assert (seen[5, 0] == 0).all()                                       # behind the source
    assert (seen[4, 0] != 0).any()                                       # in front of it


def _mutant_case(mutant):
    room = rr.room()
    if mutant in ("no_r2_clamp", "clamp_wrong_area"):
        return sr.square_case(0.05)
    if mutant in ("no_inv2pi", "w_unnormalised"):
        return sr.room_cases(0)["room/3 tilted"]
    if mutant == "cos_from_face_normal":
        return sr.room_cases(1)["room/3 tilted"]
    if mutant == "serial_sum":
        return sr.tie_case()
    if mutant == "skip_ignored":
        up = sr.unit32(np.tile([[0.0, 0.0, 1.0]], (len(rr.room_points()), 1)))
        return sr.make_case(room, 16, rr.room_points(), up, 1, eps=0.0)
    if mutant == "eps_zero":
        pts = np.array([[3.33, 0.41, -1e-5], [3.1, 2.6, -1e-5]])         # just under the floor: the floor is met inside eps
        return sr.make_case(room, 16, pts, sr.unit32(np.tile([[0.0, 0.0, 1.0]], (2, 1))), 1, eps=1e-3)
    return sr.room_cases(1)["room/16 special" if mutant == "back_face_emits" else "room/16"]


@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    c = _mutant_case(mutant)
    e = sr.emulate(c)
    sr.check(c, e["out"], e["seen"], emu=e, what="the emulation itself")
    if mutant == "area_over_K":
        m = sr.emulate(sr.make_case((c["v"], c["tr"], c["fs"], 2), 16, c["pts"], c["nrm"], 1, mutant=mutant))
    else:
        m = sr.emulate(c, mutant)
    with pytest.raises(AssertionError):
        sr.check(c, m["out"], m["seen"], emu=e, what=mutant)


def _cpu_surface(v, tr, fs, S, em):
    from esr_nerf_amd import sources
    T = torch.from_numpy
    surf = sources.Surface(T(v), T(tr), {"emission": T(em)})
    z3, z1 = torch.zeros(S, 3, dtype=torch.float64), torch.zeros(S, dtype=torch.float64)
    area = torch.tensor([float(np.cumsum(sr.face_normals(v, tr, np.flatnonzero(fs == s))[1] * 0.5)[-1]) for s in range(S)],
                        dtype=torch.float64).reshape(S)
    rep = sources.SourceReport(0.1, T(fs), torch.tensor([int((fs == s).sum()) for s in range(S)], dtype=torch.int64).reshape(S),
                               area, z3, z3, z3, z3, z1.float(), z3, z3)
    return surf, rep


@pytest.mark.parametrize("scene, samples", [("room", 1), ("room", 3), ("room", 16), ("room x4", 17), ("room x4", 64)])
def test_source_lights_match_a_direct_loop(scene, samples):
    """also with fewer faces than samples (the room's sources have 4 faces) and with Kp > samples (3 -> 4, 17 -> 32)"""
    from esr_nerf_amd import sources
    v, tr, fs, S = rr.room() if scene == "room" else sr.refined_room(4)
    em = sr.vertex_emission(v, tr, fs, 5)
    want = sr.lights(v, tr, fs, S, samples, em)
    got = sources.source_lights(*_cpu_surface(v, tr, fs, S, em), samples=samples)
    assert got.slots == sr.next_pow2(samples) and len(got) == S
    assert np.array_equal(got.n.numpy(), want["n"]) and (want["n"] == np.minimum(samples, [(fs == s).sum() for s in range(S)])).all()
    for name in ("point", "normal", "weight", "radiance", "face"):
        g = getattr(got, name).numpy()
        assert g.dtype == want[name].dtype and np.array_equal(g, want[name]), (name, np.abs(g - want[name]).max())
    used = np.arange(got.slots)[None] < want["n"][:, None]
    assert (got.weight.numpy()[~used] == 0).all() and (got.face.numpy()[~used] == -1).all() and (got.weight.numpy()[used] > 0).all()


def test_the_argument_struct_is_the_headers():
    """the fields of esr_surface_light_t in the header's order, by name and width (test_host.py holds every offset against the
    C compiler's)"""
    from esr_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    body = re.search(r"typedef struct esr_surface_light \{(.*?)\} esr_surface_light_t;", header, re.S).group(1)
    names, widths = [], []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        ctype = re.match(r"(const\s+)?(\w+)", decl).group(2)
        for part in decl[re.match(r"(const\s+)?\w+", decl).end():].split(","):
            names.append(part.replace("*", "").strip())
            widths.append(8 if "*" in part else {"int64_t": 8, "int32_t": 4, "double": 8}[ctype])
    fields = _lib.EsrSurfaceLight._fields_
    assert [f[0] for f in fields] == names
    assert [ctypes.sizeof(f[1]) for f in fields] == widths
    assert _lib.SURFACE_LIGHT_MAX_SLOTS == sr.MAX_SLOTS == 64 and "esr_surface_light" in _lib.EXPORTS
    assert _lib.ABI_VERSION == int(re.search(r"#define ESR_ABI_VERSION (\d+)", header).group(1)) >= 44


def test_python_layer_refuses_bad_inputs_before_any_launch():
    from esr_nerf_amd import sources
    v, tr, fs, S = rr.room()
    surf, rep = _cpu_surface(v, tr, fs, S, sr.vertex_emission(v, tr, fs))
    L = sources.source_lights(surf, rep, 4)
    P = 5
    pts, nrm = torch.zeros(P, 3, dtype=torch.float64), torch.zeros(P, 3)
    for samples in (0, 65):
        with pytest.raises(ValueError):
            sources.source_lights(surf, rep, samples)
    with pytest.raises(ValueError):
        sources.source_lights(surf, rep, 4, edits=[dict(sources=[0], mode="brighter")])
    with pytest.raises(ValueError):
        sources.source_lights(surf, rep, 4, edits=[dict(sources=[7], mode="off")])
    with pytest.raises(ValueError):
        sources.source_lights(surf, rep, 4, edits=[dict(sources=[0], mode="off"), dict(sources=[0], mode="i_change")])
    bad = [dict(lights=None), dict(points=pts[:, :2]), dict(points=pts.int()), dict(normals=nrm[:4]), dict(eps=0.5), dict(eps=-1.0),
           dict(wo=nrm), dict(wo=nrm, basecolor=nrm, roughness=nrm[:, 0], metallic=nrm[:3, 0]),
           dict(wo=nrm.double()[:, :2], basecolor=nrm, roughness=nrm[:, 0], metallic=nrm[:, 0]), dict(bvh="tree"),
           dict(lights=sources.SourceLights(L.point[:, :3], L.normal[:, :3], L.weight[:, :3], L.radiance[:, :3], L.face[:, :3], L.n)),
           dict(lights=sources.SourceLights(L.point.float(), L.normal, L.weight, L.radiance, L.face, L.n))]
    for kw in bad:
        args = dict(lights=L, points=pts, normals=nrm)
        args.update(kw)
        with pytest.raises(ValueError):
            sources.direct_light(surf, **args)

    class Cams:
        n_views, device, width, height = 2, torch.device("cpu"), 4, 4
    for kw in (dict(view=2), dict(view=-1), dict(view=True), dict(view=0, samples=65), dict(view=0, edits=[dict(sources=[9], mode="off")])):
        with pytest.raises(ValueError):
            sources.lit_view(surf, rep, Cams(), **kw)
    other = Cams()
    other.device = torch.device("meta")
    with pytest.raises(ValueError):
        sources.lit_view(surf, rep, other, 0)
