"""esr_surface_path_is and sources.path_light(sampling="brdf") / lit_view / bake_irradiance(paths=) on the device against
tests/surfpath_is_ref.py.

`trace`, `end` and `n_open` equal to the restatement on every path without an ambiguous decision, out within K_FAMILY 2^-24 absref
of the float64 restatement per value, bit-equal to the emulation for D = 1, mode 1, a constant environment and no source, and
exactly +0 in the components that have no light.  Every output sits between guard bytes at a pointer that is 8- but not 32-byte
aligned, one case runs on inputs that start one row into their allocation, the inputs are bit-identical afterwards, two runs
give the same bytes and so does every chunking through point_base.  The worst ratios per family are printed (-s): the constants
of surfpath_is_ref.py come from them."""
import ctypes

import numpy as np
import pytest
import torch

import surfenv_ref as sv
import surflight_ref as sr
import surfpath_is_ref as si
import surfpath_ref as sp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, FILL = 64, 0xA5
_memo = {}
WORST = {k: 0.0 for k in si.K_FAMILY}
WORST_EMU = {k: 0.0 for k in si.K_FAMILY}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def dev(x, dtype=None):
    t = torch.from_numpy(np.array(x, order="C")).to(DEV)
    return t if dtype is None else t.to(dtype)


def guarded(shape, dtype):
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    raw = torch.full((GUARD + 8 + n + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 32 == 0
    return raw, raw[GUARD + 8: GUARD + 8 + n].view(dtype).reshape(shape), n


def guards_intact(raw, n):
    return bool((raw[:GUARD + 8] == FILL).all()) and bool((raw[GUARD + 8 + n:] == FILL).all())


def shifted(x):
    """a device copy of x that starts one row into its allocation"""
    x = torch.from_numpy(np.ascontiguousarray(x))
    buf = torch.zeros((x.shape[0] + 1,) + tuple(x.shape[1:]), dtype=x.dtype, device=DEV)
    buf[1:] = x.to(DEV)
    return buf[1:]


def bvh_for(c):
    from esr_nerf_amd import raycast
    # (the memo keeps the array whose id is the key alive)
    return memo(("bvh", id(c["v"])), lambda: (raycast.build(dev(c["v"]).reshape(-1, 3), dev(c["tr"]).reshape(-1, 3)), c["v"]))[0]


def run(c, want=True, shift=False, rows=None, **over):
    """one guarded call of the C entry on a case of surfpath_is_ref -> (code, out, n_open, trace, end) as numpy.  `rows`: the
    points (a, b) of the case only, with point_base moved by a.  `over`: arguments replaced by name, or pointers dropped (drop=(...))"""
    from esr_nerf_amd import _lib
    mode, N, D, L, sg = c["mode"], c["N"], c["D"], c["L"], c["sg"]
    a, b = rows or (0, len(c["pts"]))
    P = b - a
    bvh = bvh_for(c)
    up = shifted if shift else dev
    d = dict(v_normal=up(c["attrs"]["normal"]), v_base=up(c["attrs"]["base"]), v_rough=up(c["attrs"]["rough"]), v_metal=up(c["attrs"]["metal"]),
             pts=up(c["pts"][a:b]), nrm=up(c["nrm"][a:b]))
    if L is not None:
        d.update({"l_" + k: up(L[k]) for k in ("point", "normal", "weight", "radiance", "face")})
    if sg is not None:
        d.update(mus=up(sg[0]), lambdas=up(np.asarray(sg[1]).reshape(-1)), lobes=up(sg[2]))
    if c["face"] is not None:
        d["face"] = up(c["face"][a:b])
    if mode == 0:
        d.update({k: up(c["mat"][k][a:b]) for k in ("base", "rough", "metal", "wo")})
    before = {k: x.clone() for k, x in d.items()}
    outs = dict(out=guarded((P, 3, 3), torch.float32), n_open=guarded((P,), torch.int32), trace=guarded((P, N, D), torch.int32),
                end=guarded((P, N), torch.uint8))
    drop = over.pop("drop", ())
    p = lambda k: _lib.ptr(d[k]) if k in d and k not in drop else None
    o = lambda k: _lib.ptr(outs[k][1]) if (want or k == "out") and k not in drop else None
    S, kp = (0, 1) if L is None else L["weight"].shape
    seed = c["seed"] - 2 ** 64 if c["seed"] >= 2 ** 63 else c["seed"]
    code = _lib.lib().esr_surface_path_is(
        _lib.ptr(bvh.nodes), over.get("n_faces", bvh.n_faces), _lib.ptr(bvh.vertices), over.get("n_vertices", int(bvh.vertices.shape[0])),
        _lib.ptr(bvh.triangles), p("v_normal"), p("v_base"), p("v_rough"), p("v_metal"), over.get("n_sources", S), over.get("slots", kp),
        p("l_point"), p("l_normal"), p("l_weight"), p("l_radiance"), p("l_face"), over.get("eps", float(c["eps"])), p("mus"), p("lambdas"),
        p("lobes"), over.get("n_sg", 0 if sg is None else len(sg[0])), over.get("n_points", P), p("pts"), p("nrm"), p("face"), p("base"),
        p("rough"), p("metal"), p("wo"), over.get("mode", mode), over.get("n_paths", N), over.get("depth", D), over.get("rr_start", c["rr"]),
        over.get("t_min", float(c["t_min"])), seed, over.get("point_base", c["point_base"] + a), o("out"), o("n_open"), o("trace"), o("end"),
        _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    for k, (raw, _, n) in outs.items():
        assert guards_intact(raw, n), (k, "a guard byte was written")
    for k, x in d.items():
        assert not x.numel() or torch.equal(x.view(torch.uint8), before[k].view(torch.uint8)), (k, "an input changed")
    for k, (_, t, _) in outs.items():
        if code != 0 or (k != "out" and not want):
            assert bool((t.view(torch.uint8) == FILL).all()), (k, "written by a refused call or without being asked for")
    return (code,) + tuple(outs[k][1].cpu().numpy() for k in ("out", "n_open", "trace", "end"))


def generic():
    return memo("generic", si.generic_cases)


def checked(c, out, n_open, trace, end, what, emu=None, values=True):
    emu = emu or si.emulate(c)
    worst, amb = si.check(c, out, n_open, trace, end, emu=emu, what=what, values=values)
    w_emu, _ = si.check(c, emu["out"], emu["n_open"], emu["trace"], emu["end"], emu=emu, what=what + " (emulation)", values=values)
    for fam in worst:
        WORST[fam], WORST_EMU[fam] = max(WORST[fam], worst[fam]), max(WORST_EMU[fam], w_emu[fam])
    print(f"  {what:30s} worst ratio {({k: round(x, 3) for k, x in worst.items()})} (the emulation's {({k: round(x, 3) for k, x in w_emu.items()})}), "
          f"{amb} ambiguous paths; so far {({k: round(x, 3) for k, x in WORST.items()})} / {({k: round(x, 3) for k, x in WORST_EMU.items()})}")
    return worst, amb, emu


@pytest.mark.parametrize("name", tuple(si.generic_cases()))
def test_case_against_the_restatement(name):
    c = generic()[name]
    code, out, n_open, trace, end = run(c, shift=name == "N=65")
    assert code == 0
    worst, amb, emu = checked(c, out, n_open, trace, end, name)
    assert amb == 0, "the seeds are chosen so that no decision of the restatement is ambiguous"
    assert np.array_equal(n_open, emu["n_open"]) and np.array_equal(trace, emu["trace"]) and np.array_equal(end, emu["end"])
    code2, out2, _, _, _ = run(c, want=False)
    assert code2 == 0 and np.array_equal(out.view(np.uint32), out2.view(np.uint32)), "two runs, with and without the optional outputs: the same bytes"


def test_roughness_zero():
    """kappa = 2e7 at the 1e-7 clamp: the bound says nothing there (surfpath_is_ref's docstring); trace, end, n_open and finiteness"""
    c = si.zero_rough_case()
    code, out, n_open, trace, end = run(c)
    assert code == 0 and np.isfinite(out).all()
    _, amb, emu = checked(c, out, n_open, trace, end, "roughness 0", values=False)
    assert amb == 0 and np.array_equal(trace, emu["trace"]) and np.array_equal(end, emu["end"]) and np.array_equal(n_open, emu["n_open"])
    assert (end == 4).any() and (end == 0).any()


def test_no_point_touches_nothing():
    c = si.make_case("room", 0, 4, 2, 2, 16, 48, 0, rr=1)
    code, out, *_ = run(c)
    assert code == 0 and out.shape == (0, 3, 3)
    c = si.make_case("room", 3, 4, 2, 2, 16, 48, 0, rr=1)
    every = ("v_normal", "v_base", "v_rough", "v_metal", "pts", "nrm", "l_point", "l_normal", "l_weight", "l_radiance", "l_face", "mus", "lambdas",
             "lobes", "base", "rough", "metal", "wo", "out", "n_open", "trace", "end")
    assert run(c, n_points=0, drop=every)[0] == 0


def test_a_second_grid_trip():
    """P = 8193 with N = 64: a block of 256 lanes holds 4 points and the launch cap is 2048 blocks, 8192 points a trip, so the
    last point is the second trip of block 0.  The restatement runs on every 64th point and the last two"""
    P, N = 8193, 64
    rng = np.random.default_rng(9)
    pts = np.stack([rng.uniform(0.2, 1.4, P), rng.uniform(0.2, 1.5, P), rng.uniform(0.0, 0.9, P)], 1)
    nrm = sr.unit32(rng.uniform(-1, 1, (P, 3)) + np.array([0.0, 0.0, 1.5]))
    c = si.make_case(1, P, N, 1, 0, 1, 48, 1, rr=1, seed=9, pts=pts, nrm=nrm)
    code, out, n_open, trace, end = run(c)
    assert code == 0
    sub = np.r_[np.arange(0, P, 64), P - 2, P - 1]
    cs = dict(c, pts=c["pts"][sub], nrm=c["nrm"][sub], face_nrm=c["nrm"][sub], point_ids=sub)
    checked(cs, out[sub], n_open[sub], trace[sub], end[sub], "second trip N=64")
    assert (trace >= 0).any() and (trace == -1).any() and out[-1, 0].max() > 0


def test_chunks_give_the_bytes_of_one_call():
    c = generic()["P=65"]
    whole = run(c)
    assert whole[0] == 0
    for cuts in ((0, 13, 65), (0, 64, 65), (0, 1, 33, 65)):
        parts = [run(c, rows=(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
        assert all(p[0] == 0 for p in parts)
        for k in range(1, 5):
            got = np.concatenate([p[k] for p in parts])
            assert got.tobytes() == whole[k].tobytes(), (cuts, k)
    # and the counter does hold the point: another base gives other paths
    assert not np.array_equal(run(c, point_base=7)[3], whole[3])


def test_the_roulette_starts_where_it_is_told():
    """rr_start >= depth is no roulette: the bytes of rr_start = depth, and no code 3; rr_start = 1 ends paths with code 3"""
    c = generic()["rr_start=4 mode 0"]
    base = run(c)
    for rr_start in (5, 2 ** 31 - 1):
        again = run(c, rr_start=rr_start)
        assert again[0] == 0 and all(np.array_equal(x, y) for x, y in zip(again[1:], base[1:]))
    assert not (base[4] == 3).any() and (run(generic()["rr_start=1 mode 0"])[4] == 3).any()


def test_capacity_and_bad_arguments():
    from esr_nerf_amd import _lib
    c = si.make_case("room", 3, 4, 2, 2, 16, 48, 0, rr=1)
    assert run(c)[0] == 0
    for kw in (dict(rr_start=0), dict(rr_start=-1), dict(n_paths=0), dict(n_paths=-1), dict(depth=0), dict(n_sg=-1), dict(mode=2), dict(mode=-1),
               dict(t_min=-1e-9), dict(t_min=float("nan")), dict(eps=0.5), dict(eps=-1e-9), dict(eps=float("nan")), dict(slots=0), dict(slots=3),
               dict(n_points=-1), dict(n_faces=-1), dict(n_vertices=-1), dict(n_sources=-1), dict(point_base=-1), dict(drop=("pts",)),
               dict(drop=("nrm",)), dict(drop=("base",)), dict(drop=("rough",)), dict(drop=("metal",)), dict(drop=("wo",)), dict(drop=("out",)),
               dict(drop=("v_normal",)), dict(drop=("v_base",)), dict(drop=("v_rough",)), dict(drop=("v_metal",)), dict(drop=("l_point",)),
               dict(drop=("l_normal",)), dict(drop=("l_weight",)), dict(drop=("l_radiance",)), dict(drop=("l_face",)), dict(drop=("mus",)),
               dict(drop=("lambdas",)), dict(drop=("lobes",))):
        assert run(c, **kw)[0] == _lib.EINVAL, kw
    for kw in (dict(n_paths=4097), dict(depth=9), dict(n_sg=65), dict(slots=128), dict(n_points=2 ** 31), dict(n_faces=2 ** 31),
               dict(n_vertices=2 ** 31), dict(n_sources=2 ** 31), dict(point_base=2 ** 32 - 2)):
        assert run(c, **kw)[0] == _lib.ECAP, kw
    assert run(c, point_base=2 ** 32 - 3)[0] == 0
    # a misaligned pointer: the float64 points one float in
    bvh = bvh_for(c)
    x = dev(np.zeros(48, np.float32))
    odd, ok = ctypes.c_void_p(x.data_ptr() + 4), _lib.ptr(x)
    code = _lib.lib().esr_surface_path_is(_lib.ptr(bvh.nodes), 0, None, 0, None, None, None, None, None, 0, 1, None, None, None, None, None, 1e-6,
                                          None, None, None, 0, 1, odd, ok, None, None, None, None, None, 1, 1, 1, 1, 1e-6, 0, 0, ok, None, None,
                                          None, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert code == _lib.EINVAL and float(x.abs().max()) == 0.0
    # mode 1 needs no material at the points; no source and no environment need no arrays
    c1 = si.make_case("room", 3, 4, 2, 0, 1, 0, 1, rr=1)
    assert run(c1, drop=("base", "rough", "metal", "wo"))[0] == 0


# ----------------------------------------------------------------------------------------------------------------------
# the Python layer


class Report:
    """what source_lights reads of a SourceReport"""
    def __init__(self, face_source, n, v, tr):
        fs = face_source.cpu().numpy()
        self.face_source, self.n = face_source, n
        self.area = dev(np.array([float(np.cumsum(sr.face_normals(v, tr, np.flatnonzero(fs == s))[1] * 0.5)[-1]) for s in range(n)]).reshape(n))

    def __len__(self):
        return self.n


def _surface(name, seed=0):
    from esr_nerf_amd import sources
    (v, tr, fs, S), _ = sp.scene(name)
    attrs = si.attrs_is(name)
    em = sr.vertex_emission(v, tr, fs, seed)
    surf = sources.Surface(dev(v), dev(tr), dict(normal=dev(attrs["normal"]), basecolor=dev(attrs["base"]), roughness=dev(attrs["rough"]),
                                                 metallic=dev(attrs["metal"]), emission=dev(em), sdf=dev(np.zeros(len(v), np.float32))))
    return surf, Report(dev(fs), S, v, tr), (v, tr, fs, S), attrs, em


@pytest.mark.parametrize("mode, roulette", [(0, None), (0, 1), (1, 2)])
def test_path_light_is_the_abi_call(mode, roulette):
    """path_light(sampling="brdf") on the room with a window: the dict is the C entry's output, a small chunk gives the same
    bytes, and the default sampling still gives section X's"""
    from esr_nerf_amd import sources
    surf, rep, (v, tr, fs, S), attrs, em = _surface("window", 3)
    c = si.make_case("window", 33, 8, 3, 1, 16, 48, mode, rr=roulette, seed=40 + mode)
    c["L"] = sr.lights(v, tr, fs, S, 16, em)
    c["face"] = np.full(33, -1, np.int32)
    kw = dict(env=tuple(dev(x) for x in c["sg"]), paths=8, depth=3, samples=16, seed=c["seed"], mode=mode, bvh=bvh_for(c), t_min=c["t_min"],
              eps=c["eps"], faces=dev(c["face"]))
    if mode == 0:
        kw.update(basecolor=dev(c["mat"]["base"]), roughness=dev(c["mat"]["rough"]), metallic=dev(c["mat"]["metal"]), wo=dev(c["mat"]["wo"]))
    got = sources.path_light(surf, rep, dev(c["pts"]), dev(c["nrm"]), return_trace=True, sampling="brdf", roulette=roulette, **kw)
    code, out, n_open, trace, end = run(c)
    assert code == 0 and set(got) == {"env_dir", "env_indir", "src_indir", "open", "trace", "end"}
    for i, k in enumerate(sp.COMPONENTS):
        assert got[k].dtype == torch.float32 and np.array_equal(got[k].cpu().numpy().view(np.uint32), out[:, i].view(np.uint32)), k
    assert np.array_equal(got["trace"].cpu().numpy(), trace) and np.array_equal(got["end"].cpu().numpy(), end)
    assert np.array_equal(got["open"].cpu().numpy(), n_open.astype(np.float32) / np.float32(8))
    checked(c, out, n_open, trace, end, f"path_light mode {mode} roulette {roulette}")
    small = sources.path_light(surf, rep, dev(c["pts"]), dev(c["nrm"]), chunk=7, sampling="brdf", roulette=roulette, **kw)
    assert set(small) == {"env_dir", "env_indir", "src_indir", "open"}
    for k in small:
        assert torch.equal(small[k], got[k]), k
    assert float(got["env_indir"].max()) > 0 and float(got["src_indir"].max()) > 0
    plain = sources.path_light(surf, rep, dev(c["pts"]), dev(c["nrm"]), **kw)
    named = sources.path_light(surf, rep, dev(c["pts"]), dev(c["nrm"]), sampling="uniform", **kw)
    assert all(torch.equal(plain[k], named[k]) for k in plain) and not torch.equal(plain["env_dir"], got["env_dir"])
    with pytest.raises(ValueError):
        sources.path_light(surf, rep, dev(c["pts"]), dev(c["nrm"]), roulette=1, **kw)


def _camera(eye, target, up, f, width, height):
    from esr_nerf_amd.camera import Cameras
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    pose = np.stack([right, np.cross(fwd, right), fwd, eye], 1).astype(np.float32)
    return Cameras(torch.from_numpy(pose[None]).to(DEV), f, f - 1.0, width * 0.5 - 0.3, height * 0.5 + 0.2, width, height)


def test_lit_view_in_the_room():
    """lit_view(paths=, sampling="brdf") in the room with a window: the parent's keys keep their bytes, the new ones are
    path_light's at the pixels' points, finite and not negative"""
    from esr_nerf_amd import raycast, sources
    surf, rep, _, _, _ = _surface("window", 2)
    cams = _camera([3.4, 2.5, 1.3], [0.9, 1.2, 1.5], [0.0, 0.0, 1.0], 17.0, 24, 16)
    env = tuple(dev(x) for x in sv.sg_random(48, 8))
    H, W = cams.height, cams.width
    bvh = raycast.build(surf.vertices, surf.triangles)
    plain = sources.lit_view(surf, rep, cams, 0, samples=16, bvh=bvh)
    uniform = sources.lit_view(surf, rep, cams, 0, samples=16, bvh=bvh, env=env, paths=4, depth=3, seed=11)
    traced = sources.lit_view(surf, rep, cams, 0, samples=16, bvh=bvh, env=env, paths=4, depth=3, seed=11, sampling="brdf", roulette=1)
    assert set(traced) == set(uniform) == set(plain) | {"lin/env_dir", "lin/env_indir", "lin/src_indir", "etc/open"}
    for k in plain:
        assert torch.equal(plain[k].view(torch.uint8), traced[k].view(torch.uint8)), k
    o, d, _ = raycast.pixel_rays(cams, 0)
    hit = raycast.cast(bvh, o, d)
    x, normal, a, wo = sources._hit_points(surf, hit, d)
    got = hit.face >= 0
    at = (x, normal, hit.face, a["basecolor"], a["roughness"][:, 0], a["metallic"][:, 0], wo)
    zero = torch.zeros(1, 3, dtype=torch.float32, device=DEV)
    for chunk in (sources.PATH_CHUNK, 37):
        lit = sources.path_light(surf, rep, *at, env=env, paths=4, depth=3, samples=16, seed=11, bvh=bvh, sampling="brdf", roulette=1, chunk=chunk)
        for k in sp.COMPONENTS:
            assert torch.equal(traced["lin/" + k], torch.where(got[:, None], lit[k], zero).reshape(H, W, 3)), (k, chunk)
            assert bool(torch.isfinite(traced["lin/" + k]).all()) and float(traced["lin/" + k].min()) >= 0.0
        assert torch.equal(traced["etc/open"], torch.where(got, lit["open"], zero[0, 0]).reshape(H, W))
    assert float(traced["lin/env_dir"].max()) > 0 and float(traced["lin/env_indir"].max()) > 0 and float(traced["lin/src_indir"].max()) > 0
    assert not torch.equal(traced["lin/env_dir"], uniform["lin/env_dir"])
    with pytest.raises(ValueError):
        sources.lit_view(surf, rep, cams, 0, env=env, sampling="brdf")


def test_bake_irradiance_with_paths():
    """bake_irradiance(paths=) in the room with a window: the keys without paths keep their bytes, light/paths is mode 1 of the
    entry at the texels whose centre lies in their face, the same bytes under every chunking, 0 elsewhere"""
    from esr_nerf_amd import atlas, raycast, sources
    surf, rep, (v, tr, fs, S), _, _ = _surface("window", 2)
    env = tuple(dev(x) for x in sv.sg_random(48, 8))
    at = atlas.build(surf.vertices, surf.triangles, size=256)
    bvh = raycast.build(surf.vertices, surf.triangles)
    plain = sources.bake_irradiance(surf, at, rep, samples=8, env=env, env_dirs=16, bvh=bvh)
    assert set(plain) == {"light/sources", "light/env"}
    baked = sources.bake_irradiance(surf, at, rep, samples=8, env=env, env_dirs=16, bvh=bvh, paths=8, depth=3, seed=5, roulette=2)
    assert set(baked) == set(plain) | {"light/paths"}
    for k in plain:
        assert torch.equal(plain[k].view(torch.uint8), baked[k].view(torch.uint8)), k
    lp = baked["light/paths"]
    assert lp.dtype == torch.float32 and tuple(lp.shape) == (256, 256, 3, 3) and bool(torch.isfinite(lp).all()) and float(lp.min()) >= 0.0
    inside = (at.flags & 1) != 0
    assert float(lp[~inside].abs().max()) == 0.0 and all(float(lp[:, :, i].max()) > 0 for i in range(3))
    for chunk in (500, 61):
        again = sources.bake_irradiance(surf, at, rep, samples=8, env=env, env_dirs=16, bvh=bvh, paths=8, depth=3, seed=5, roulette=2, chunk=chunk)
        assert torch.equal(again["light/paths"].view(torch.uint8), lp.view(torch.uint8)), chunk
    idx = torch.nonzero(inside.reshape(-1)).reshape(-1)
    face = at.face.reshape(-1)[idx].contiguous()
    lit = sources.path_light(surf, rep, at.point.reshape(-1, 3)[idx].double(), sources.face_normals(surf)[face.long()], face, env=env, paths=8, depth=3,
                             samples=8, seed=5, mode=1, bvh=bvh, sampling="brdf", roulette=2)
    assert torch.equal(lp.reshape(-1, 3, 3)[idx], torch.stack([lit[k] for k in sp.COMPONENTS], 1))
    no_env = sources.bake_irradiance(surf, at, rep, samples=8, bvh=bvh, paths=8, depth=3, seed=5, roulette=2)
    assert set(no_env) == {"light/sources", "light/paths"} and float(no_env["light/paths"][:, :, :2].abs().max()) == 0.0
    assert torch.equal(no_env["light/paths"][:, :, 2], lp[:, :, 2])
