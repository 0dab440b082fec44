"""esr_surface_env and sources.environment_light / vertex_env_radiance / lit_view on the device against tests/surfenv_ref.py.

`hit` equal to the brute force on every unambiguous ray, `n_open` exact where no direction is ambiguous, out within
K_FAMILY 2^-24 absref of the float64 restatement per value, and bit-equal to the emulation where the environment is a constant
without a mesh.  Every output sits between guard bytes at a pointer that is 8- but not 32-byte aligned, one case runs on inputs
that start one row into their allocation, the inputs are bit-identical afterwards and two runs give the same bytes.  The worst
ratios per family are printed (-s): the constants of surfenv_ref.py come from them."""
import ctypes

import numpy as np
import pytest
import torch

import raycast_ref as rr
import surfenv_ref as sv
import surflight_ref as sr
from conftest import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, FILL = 64, 0xA5
_memo = {}
WORST = {k: 0.0 for k in sv.K_FAMILY}


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


def run(c, want_open=True, want_hit=True, shift=False, **over):
    """one guarded call of the C entry on a case of surfenv_ref -> (code, out, n_open, hit) as numpy.  `over`: arguments
    replaced by name (n_dirs, n_sg, mode, t_min, n_points, n_faces, n_vertices) or pointers dropped (drop=("dirs", ...))"""
    from esr_nerf_amd import _lib
    mode = c["mode"]
    P, R, J = len(c["pts"]), len(c["dirs"]), len(c["sg"][0])
    bvh = bvh_for(c)
    up = shifted if shift else dev
    d = dict(dirs=up(c["dirs"]), mus=up(c["sg"][0]), lambdas=up(np.asarray(c["sg"][1]).reshape(-1)), lobes=up(c["sg"][2]),
             pts=up(c["pts"]), nrm=up(c["nrm"]))
    if c["vrad"] is not None:
        d["vrad"] = up(c["vrad"])
    if c["face"] is not None:
        d["face"] = up(c["face"])
    if mode == 0:
        d.update({k: up(c["mat"][k]) for k in ("base", "rough", "metal", "wo")})
    before = {k: x.clone() for k, x in d.items()}
    raw_o, out, n_o = guarded((P, 3), torch.float32)
    raw_n, n_open, n_n = guarded((P,), torch.int32)
    raw_h, hit, n_h = guarded((P, R), torch.uint8)
    drop = over.pop("drop", ())
    p = lambda k: _lib.ptr(d[k]) if k in d and k not in drop else None
    code = _lib.lib().esr_surface_env(
        _lib.ptr(bvh.nodes), over.get("n_faces", bvh.n_faces), _lib.ptr(bvh.vertices), over.get("n_vertices", int(bvh.vertices.shape[0])),
        _lib.ptr(bvh.triangles), p("dirs"), over.get("n_dirs", R), p("mus"), p("lambdas"), p("lobes"), over.get("n_sg", J), p("vrad"),
        over.get("n_points", P), p("pts"), p("nrm"), p("face"), p("base"), p("rough"), p("metal"), p("wo"), over.get("mode", mode),
        over.get("t_min", float(c["t_min"])), None if "out" in drop else _lib.ptr(out), _lib.ptr(n_open) if want_open else None,
        _lib.ptr(hit) if want_hit else None, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert guards_intact(raw_o, n_o) and guards_intact(raw_n, n_n) and guards_intact(raw_h, n_h), "a guard byte was written"
    for k, x in d.items():
        assert not x.numel() or torch.equal(x.view(torch.uint8), before[k].view(torch.uint8)), (k, "an input changed")
    if code != 0 or not want_hit:
        assert bool((hit.view(torch.uint8) == FILL).all()), "hit written without being asked for"
    if code != 0 or not want_open:
        assert bool((n_open.view(torch.uint8) == FILL).all()), "n_open written without being asked for"
    if code != 0:
        assert bool((out.view(torch.uint8) == FILL).all()), "out written by a refused call"
    return code, out.cpu().numpy(), n_open.cpu().numpy(), hit.cpu().numpy()


def generic():
    return memo("generic", sv.generic_cases)


def checked(c, out, n_open, hit, what, emu=None):
    emu = emu or sv.emulate(c)
    worst, amb = sv.check(c, out, n_open, hit, emu=emu, what=what)
    w_emu, _ = sv.check(c, emu["out"], emu["n_open"], emu["hit"], emu=emu, what=what + " (emulation)")
    fam = sv.family(c)
    WORST[fam] = max(WORST[fam], worst)
    print(f"  {what:40s} {fam:18s} worst ratio {worst:.3f} (the emulation's {w_emu:.3f}), {amb} ambiguous directions; so far {WORST}")
    return worst, amb, emu


@pytest.mark.parametrize("name", tuple(sv.generic_cases()))
def test_case_against_the_restatement(name):
    c = generic()[name]
    code, out, n_open, hit = run(c, shift=name == "R=17 mode 0 +radiance")
    assert code == 0
    worst, amb, emu = checked(c, out, n_open, hit, name)
    assert amb == 0
    assert np.array_equal(n_open, emu["n_open"]) and np.array_equal(hit, emu["hit"])
    code2, out2, _, _ = run(c, want_open=False, want_hit=False)
    assert code2 == 0 and np.array_equal(out.view(np.uint32), out2.view(np.uint32)), "two runs, with and without n_open and hit: the same bytes"
    if name == "tie":
        assert out[0, 0] != sv.emulate(c, "serial_sum")["out"][0, 0], "the lane-strided butterfly order"
    if name == "t_min met exactly":
        assert n_open[0] == 1
    if name == "slab":
        assert n_open[0] == 0 and (out == 0).all()


@pytest.mark.parametrize("name", tuple(sv.constructed_cases()))
def test_constructed_ambiguity(name):
    c, allowed = sv.constructed_cases()[name]
    code, out, n_open, hit = run(c)
    assert code == 0
    _, amb, emu = checked(c, out, n_open, hit, name)
    assert amb >= 1 and not (emu["ambiguous"] & ~allowed).any()


def test_no_point_touches_nothing():
    c = sv.shape_case(0, 16, 48, "room", 0, True)
    code, out, n_open, hit = run(c)
    assert code == 0 and out.shape == (0, 3)
    c = sv.shape_case(3, 16, 48, "room", 0, True)
    assert run(c, n_points=0, drop=("dirs", "mus", "lambdas", "lobes", "pts", "nrm", "base", "rough", "metal", "wo", "out"))[0] == 0


def test_a_second_grid_trip():
    """P = 8193 at Kd = 64: a block of 256 lanes holds 4 points and the launch cap is 2048 blocks, 2048 * 4 = 8192 points a trip,
    so the last point is the second trip of block 0.  The restatement runs on every 16th point and the last two"""
    P = 8193
    rng = np.random.default_rng(9)
    pts = np.stack([rng.uniform(0.2, 1.4, P), rng.uniform(0.2, 1.5, P), rng.uniform(0.0, 0.9, P)], 1)
    nrm = sr.unit32(rng.uniform(-1, 1, (P, 3)) + np.array([0.0, 0.0, 1.5]))
    c = sv.make_case(sv.one_face(), 64, sv.sg_random(48, 9), pts, nrm, 1, vrad=True, seed=9)
    code, out, n_open, hit = run(c)
    assert code == 0
    sub = np.r_[np.arange(0, P, 16), P - 2, P - 1]
    cs = dict(c, pts=pts[sub], nrm=nrm[sub], face_nrm=nrm[sub])
    _, amb, emu = checked(cs, out[sub], n_open[sub], hit[sub], "second trip")
    assert (hit[-1] == 1).any() or (n_open[-1] == 64)
    assert (hit == 1).any() and (n_open < 64).any() and out[-1].max() > 0


def test_capacity_and_bad_arguments():
    from esr_nerf_amd import _lib
    c = sv.shape_case(3, 16, 48, "room", 0, True)
    assert run(c)[0] == 0
    for kw in (dict(n_dirs=0), dict(n_dirs=-1), dict(n_sg=0), dict(mode=2), dict(mode=-1), dict(t_min=-1e-9), dict(t_min=float("nan")),
               dict(n_points=-1), dict(n_faces=-1), dict(n_vertices=-1), dict(drop=("dirs",)), dict(drop=("mus",)), dict(drop=("lambdas",)),
               dict(drop=("lobes",)), dict(drop=("pts",)), dict(drop=("nrm",)), dict(drop=("base",)), dict(drop=("rough",)),
               dict(drop=("metal",)), dict(drop=("wo",)), dict(drop=("out",))):
        assert run(c, **kw)[0] == _lib.EINVAL, kw
    for kw in (dict(n_dirs=4097), dict(n_sg=65), dict(n_points=2 ** 31), dict(n_faces=2 ** 31), dict(n_vertices=2 ** 31)):
        assert run(c, **kw)[0] == _lib.ECAP, kw
    # a misaligned pointer: the float64 points one float in
    bvh = bvh_for(c)
    x = dev(np.zeros(48, np.float32))
    odd, ok = ctypes.c_void_p(x.data_ptr() + 4), _lib.ptr(x)
    code = _lib.lib().esr_surface_env(_lib.ptr(bvh.nodes), bvh.n_faces, _lib.ptr(bvh.vertices), int(bvh.vertices.shape[0]),
                                      _lib.ptr(bvh.triangles), ok, 16, ok, ok, ok, 1, None, 1, odd, ok, None, None, None, None, None, 1,
                                      1e-6, ok, None, None, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert code == _lib.EINVAL and float(x.abs().max()) == 0.0
    # mode 1 needs no material
    c1 = sv.shape_case(3, 16, 48, "room", 1, False)
    assert run(c1, drop=("base", "rough", "metal", "wo"))[0] == 0


# ----------------------------------------------------------------------------------------------------------------------
# the Python layer


def _env(c):
    return tuple(dev(x) for x in c["sg"])


def _surface(v, tr, seed=0):
    from esr_nerf_amd import sources
    rng = np.random.default_rng(seed + 50)
    V = len(v)
    nv, ln = sr.face_normals(v, tr, np.arange(len(tr)))
    vn = np.zeros((V, 3))
    mid = v.mean(0)
    for f in range(len(tr)):
        n = nv[f] / ln[f]
        vn[tr[f]] = -n if ((mid - v[tr[f, 0]]) * n).sum() < 0 else n      # (the room's quads own their vertices)
    attrs = dict(normal=sr.unit32(vn + 0.05 * rng.uniform(-1, 1, (V, 3))), basecolor=rng.uniform(0.1, 0.9, (V, 3)).astype(np.float32),
                 roughness=rng.uniform(0.2, 0.9, V).astype(np.float32), metallic=rng.uniform(0, 1, V).astype(np.float32),
                 emission=np.zeros((V, 3), np.float32), sdf=np.zeros(V, np.float32))
    return sources.Surface(dev(v), dev(tr), {k: dev(x) for k, x in attrs.items()}), attrs


def test_environment_light_is_the_abi_call():
    from esr_nerf_amd import sources
    for mode, vrad in sv.COMBOS:
        c = sv.shape_case(33, 17, 48, "room", mode, vrad)
        c["face"] = np.full(33, -1, np.int32)
        surf, _ = _surface(c["v"], c["tr"])
        kw = dict(dirs=dev(c["dirs"]), faces=dev(c["face"]), vertex_radiance=None if c["vrad"] is None else dev(c["vrad"]),
                  bvh=bvh_for(c), t_min=c["t_min"])
        if mode == 0:
            kw.update(basecolor=dev(c["mat"]["base"]), roughness=dev(c["mat"]["rough"]), metallic=dev(c["mat"]["metal"]), wo=dev(c["mat"]["wo"]))
        got, share, hit = sources.environment_light(surf, _env(c), dev(c["pts"]), dev(c["nrm"]), return_open=True, return_hit=True, **kw)
        code, out, n_open, hit_c = run(c)
        assert code == 0 and got.dtype == torch.float32 and share.dtype == torch.float32 and hit.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy().view(np.uint32), out.view(np.uint32)) and np.array_equal(hit.cpu().numpy(), hit_c)
        assert np.array_equal(share.cpu().numpy(), n_open.astype(np.float32) / np.float32(17))
        alone = sources.environment_light(surf, _env(c), dev(c["pts"]), dev(c["nrm"]), **kw)
        assert torch.equal(alone, got)
    # a count instead of a table is hemisphere_directions; no point is no launch
    c = sv.shape_case(9, 16, 48, "room", 1, False)
    surf, _ = _surface(c["v"], c["tr"])
    a = sources.environment_light(surf, _env(c), dev(c["pts"]), dev(c["nrm"]), dirs=16)
    b = sources.environment_light(surf, _env(c), dev(c["pts"]), dev(c["nrm"]), dirs=sources.hemisphere_directions(16, DEV))
    assert torch.equal(a, b) and float(a.max()) > 0
    assert tuple(sources.environment_light(surf, _env(c), dev(c["pts"])[:0], dev(c["nrm"])[:0]).shape) == (0, 3)
    with pytest.raises(ValueError):
        sources.environment_light(surf, _env(c), dev(c["pts"]).cpu(), dev(c["nrm"]))


def test_nothing_of_size_points_times_directions_is_allocated():
    from esr_nerf_amd import sources
    P, R = 65536, 128
    c = sv.shape_case(7, 16, 48, "room", 0, False)
    surf, _ = _surface(c["v"], c["tr"])
    rng = np.random.default_rng(3)
    pts = dev(np.stack([rng.uniform(0.2, 3.8, P), rng.uniform(0.2, 2.8, P), rng.uniform(2.6, 4.0, P)], 1))
    nrm = dev(sr.unit32(rng.uniform(-1, 1, (P, 3))))
    mat = dict(basecolor=dev(rng.uniform(0.1, 0.9, (P, 3)).astype(np.float32)), roughness=dev(rng.uniform(0.2, 0.9, P).astype(np.float32)),
               metallic=dev(rng.uniform(0, 1, P).astype(np.float32)), wo=nrm)
    env, table, bvh = _env(c), sources.hemisphere_directions(R, DEV), bvh_for(c)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, share = sources.environment_light(surf, env, pts, nrm, dirs=table, bvh=bvh, return_open=True, **mat)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    outputs = P * 3 * 4 + 2 * P * 4                                       # out, n_open and the share computed from it
    print(f"  P = {P}, R = {R}: peak {peak} bytes over the start, outputs {outputs}, P R = {P * R}")
    assert peak - outputs < 1 << 20
    assert bool(torch.isfinite(out).all()) and float(share.min()) >= 0 and float(share.max()) <= 1 and float(out.max()) > 0


def test_rotating_the_lobes_is_rotating_the_scene_the_other_way():
    """environment_light with the lobes turned by a rotation Q equals the light, under the first lobes, of the scene (mesh,
    points, normals, view directions, table) turned by Q^T.  Q is the cyclic permutation of the axes (x, y, z) -> (z, x, y): a
    rotation that rounds nothing, so the two are ONE quantity computed in two orders, and the first lies inside the bound of
    the second's restatement"""
    from esr_nerf_amd import sources
    fwd, back = (lambda x: np.ascontiguousarray(np.asarray(x)[..., [2, 0, 1]])), (lambda x: np.ascontiguousarray(np.asarray(x)[..., [1, 2, 0]]))
    c = sv.shape_case(12, 64, 48, "room", 0, False)
    mus, lam, lobes = c["sg"]
    surf, _ = _surface(c["v"], c["tr"])
    got, share, hit = sources.environment_light(surf, (dev(mus), dev(lam), dev(fwd(lobes))), dev(c["pts"]), dev(c["nrm"]), dev(c["mat"]["base"]),
                                                dev(c["mat"]["rough"]), dev(c["mat"]["metal"]), dev(c["mat"]["wo"]), dirs=dev(c["dirs"]),
                                                bvh=bvh_for(c), return_open=True, return_hit=True)
    c2 = dict(c, v=back(c["v"]), pts=back(c["pts"]), nrm=back(c["nrm"]), face_nrm=back(c["nrm"]), dirs=back(c["dirs"]),
              mat=dict(c["mat"], wo=back(c["mat"]["wo"])))
    n_open = np.rint(share.cpu().numpy().astype(np.float64) * 64).astype(np.int32)
    worst, amb, emu2 = checked(c2, got.cpu().numpy(), n_open, hit.cpu().numpy(), "lobes turned against the scene turned back")
    assert amb == 0 and float(got.max()) > 0
    # and it is an edit: the light differs from the first environment's
    plain = sources.environment_light(surf, (dev(mus), dev(lam), dev(lobes)), dev(c["pts"]), dev(c["nrm"]), dev(c["mat"]["base"]),
                                      dev(c["mat"]["rough"]), dev(c["mat"]["metal"]), dev(c["mat"]["wo"]), dirs=dev(c["dirs"]), bvh=bvh_for(c))
    assert not torch.equal(plain, got)


def _vertex_case(v, tr, attrs, sg, table):
    unit = lambda x: x / np.maximum(np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]), x.dtype.type(1e-12))[:, None]
    n = unit(attrs["normal"].astype(np.float32))
    c = sv.make_case((v, tr), table, sg, v, n, 0)
    c["mat"] = dict(base=attrs["basecolor"].reshape(-1, 3), rough=attrs["roughness"].reshape(-1), metal=attrs["metallic"].reshape(-1), wo=n)
    return c


def test_vertex_env_radiance_against_the_restatement():
    from esr_nerf_amd import sources
    v, tr = sv.room()
    surf, attrs = _surface(v, tr, 4)
    sg = sv.sg_random(48, 4)
    # (the table's last direction has y == 0 exactly and runs along the room's grid lines from its vertices: the table turned)
    table = dev(sv.turned(sources.hemisphere_directions(64).numpy()))
    got = sources.vertex_env_radiance(surf, tuple(dev(x) for x in sg), table)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(v), 3)
    c = _vertex_case(v, tr, attrs, sg, table.cpu().numpy())
    emu = sv.emulate(c)
    clear = ~emu["ambiguous"].any(1)
    worst, amb = sv.check(c, got.cpu().numpy(), emu=emu, what="vertex radiance")
    WORST["reflect"] = max(WORST["reflect"], worst)
    print(f"  vertex radiance: {len(v)} vertices, {int(clear.sum())} without an ambiguous direction, worst ratio {worst:.3f}")
    assert clear.sum() >= len(v) // 4 and float(got.max()) > 0
    env = tuple(dev(x) for x in sg)
    assert torch.equal(sources.vertex_env_radiance(surf, env, 64), sources.vertex_env_radiance(surf, env, sources.hemisphere_directions(64, DEV)))


def _camera(eye, target, up, f, width, height):
    from esr_nerf_amd.camera import Cameras
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    pose = np.stack([right, np.cross(fwd, right), fwd, eye], 1).astype(np.float32)
    return Cameras(torch.from_numpy(pose[None]).to(DEV), f, f - 1.0, width * 0.5 - 0.3, height * 0.5 + 0.2, width, height), pose


def _check_lit_view(surf, rep, attrs, v, tr, cams, pose, sg, R, what):
    """lit_view with env=None against the recipe it had before the environment, and with env and bounces 0, 1 against the
    restatement at 257 pixels"""
    from esr_nerf_amd import raycast, sources
    H, W = cams.height, cams.width
    bvh = raycast.build(surf.vertices, surf.triangles)
    env = tuple(dev(x) for x in sg)
    plain = sources.lit_view(surf, rep, cams, 0, samples=16, bvh=bvh)
    assert set(plain) == {"lin/reflect", "lin/emit", "face", "depth"}
    # the recipe as it stood: cast, interpolate, direct_light
    o, d, _ = raycast.pixel_rays(cams, 0)
    hit = raycast.cast(bvh, o, d)
    x, normal, a, wo = sources._hit_points(surf, hit, d)
    reflect = sources.direct_light(surf, sources.source_lights(surf, rep, 16), x, normal, a["basecolor"], a["roughness"][:, 0], a["metallic"][:, 0], wo, bvh=bvh)
    got = hit.face >= 0
    assert torch.equal(plain["lin/reflect"], torch.where(got[:, None], reflect, torch.zeros_like(reflect)).reshape(H, W, 3))
    assert torch.equal(plain["face"], hit.face.reshape(H, W)) and torch.equal(plain["depth"], hit.t.reshape(H, W))
    one = sources.lit_view(surf, rep, cams, 0, samples=16, bvh=bvh, env=env, env_dirs=R)
    two = sources.lit_view(surf, rep, cams, 0, samples=16, bvh=bvh, env=env, env_dirs=R, bounces=1)
    assert set(one) == set(plain) | {"lin/env_dir", "etc/open"} and set(two) == set(one) | {"lin/env_indir"}
    for k in plain:
        assert torch.equal(plain[k].view(torch.uint8), one[k].view(torch.uint8)) and torch.equal(plain[k].view(torch.uint8), two[k].view(torch.uint8)), k
    assert torch.equal(one["lin/env_dir"], two["lin/env_dir"]) and torch.equal(one["etc/open"], two["etc/open"])
    share = one["etc/open"].cpu().numpy()
    assert share.dtype == np.float32 and share.shape == (H, W) and share.min() >= 0.0 and share.max() <= 1.0
    # 257 pixels against the restatement
    pix = np.unique(np.linspace(0, H * W - 1, 257).astype(np.int64))
    assert len(pix) == 257
    m = pose.astype(np.float64)
    px = ((np.arange(W) + 0.5) - cams.cx) / cams.fx
    py = ((np.arange(H) + 0.5) - cams.cy) / cams.fy
    dd = ((px[None, :, None] * m[None, None, :, 0] + py[:, None, None] * m[None, None, :, 1]) + m[None, None, :, 2]).reshape(-1, 3)[pix]
    b = rr.brute(v, tr, np.broadcast_to(m[:, 3], dd.shape), dd)
    seen = b["face"] >= 0
    f = np.maximum(b["face"], 0)
    w64 = np.stack([(1.0 - b["u"]) - b["v"], b["u"], b["v"]], 1)
    w32 = w64.astype(np.float32)
    at = lambda x, w: (x[tr[f, 0]] * w[:, 0:1] + x[tr[f, 1]] * w[:, 1:2]) + x[tr[f, 2]] * w[:, 2:3]
    unit = lambda x: x / np.maximum(np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]), x.dtype.type(1e-12))[:, None]
    A = {k: at(attrs[k].reshape(len(v), -1), w32) for k in ("normal", "basecolor", "roughness", "metallic")}
    table = sources.hemisphere_directions(R).numpy()
    c = sv.make_case((v, tr), table, sg, np.where(seen[:, None], at(v, w64), np.nan), unit(A["normal"]), 0, face=b["face"].astype(np.int32))
    c["mat"] = dict(base=A["basecolor"], rough=A["roughness"][:, 0], metal=A["metallic"][:, 0], wo=(-unit(dd)).astype(np.float32))
    emu = sv.emulate(c)
    clear = ~(b["ambiguous"] | emu["ambiguous"].any(1))
    v1, a1 = sv.reference(c, emu)
    g1 = one["lin/env_dir"].cpu().numpy().reshape(-1, 3)[pix].astype(np.float64)
    K1, K2 = sv.K_FAMILY["reflect"], sv.K_FAMILY["reflect+radiance"]
    ok = clear & seen
    r1 = np.abs(g1 - v1) / np.maximum(sv.U24 * a1, 1e-300)
    assert (r1[ok] <= K1).all(), float(r1[ok].max())
    assert (g1[~seen & clear] == 0).all() and (share.reshape(-1)[pix][~seen & clear] == 0).all()
    assert np.array_equal(share.reshape(-1)[pix][ok], (emu["n_open"].astype(np.float32) / np.float32(R))[ok])
    # one more bounce: the vertex radiance is the product's (held against the restatement on its own), the gather is restated
    vrad = sources.vertex_env_radiance(surf, env, R, bvh=bvh).cpu().numpy()
    c2 = dict(c, vrad=vrad)
    emu2 = sv.emulate(c2)
    v2, a2 = sv.reference(c2, emu2)
    g2 = two["lin/env_indir"].cpu().numpy().reshape(-1, 3)[pix].astype(np.float64)
    want = v2 - v1
    bound = sv.U24 * (K2 * a2 + K1 * a1 + np.abs(want))                    # (both launches' bounds and the subtraction's rounding)
    ok2 = ok & ~emu2["ambiguous"].any(1)
    r2 = np.abs(g2 - want) / np.maximum(bound, 1e-300)
    assert (r2[ok2] <= 1).all(), float(r2[ok2].max())
    assert (g2[~seen & clear] == 0).all()
    print(f"  {what}: {int(seen.sum())} of 257 pixels hit, {int((~clear).sum())} ambiguous, open share up to {share.max():.3f}, "
          f"env_dir worst ratio {float(r1[ok].max()) if ok.any() else 0:.3f}, env_indir err / bound {float(r2[ok2].max()) if ok2.any() else 0:.3f}, "
          f"env_dir max {g1.max():.4f}, env_indir max {g2.max():.4f}")
    assert ok.sum() > 40 and ok2.sum() > 40
    return one, two


class Report:
    """what source_lights reads of a SourceReport"""
    def __init__(self, face_source, n, v, tr):
        fs = face_source.cpu().numpy()
        self.face_source, self.n = face_source, n
        self.area = dev(np.array([float(np.cumsum(sr.face_normals(v, tr, np.flatnonzero(fs == s))[1] * 0.5)[-1]) for s in range(n)]).reshape(n))

    def __len__(self):
        return self.n


def test_lit_view_in_the_room():
    """the room with a window: the ceiling patch's faces are taken out, so that the sky is seen from inside"""
    v, tr, fs, S = sr.refined_room(2)
    keep = fs != 0
    tr, fs = tr[keep], np.where(fs[keep] == 1, 0, -1).astype(np.int32)
    surf, attrs = _surface(v, tr, 2)
    attrs["emission"] = sr.vertex_emission(v, tr, fs, 2)
    surf.attrs["emission"] = dev(attrs["emission"])
    cams, pose = _camera([3.4, 2.5, 1.3], [0.9, 1.2, 1.5], [0.0, 0.0, 1.0], 17.0, 24, 16)
    one, two = _check_lit_view(surf, Report(dev(fs), 1, v, tr), attrs, v, tr, cams, pose, sv.sg_random(48, 8), 128, "room with a window")
    assert float(one["lin/env_dir"].max()) > 0 and float(two["lin/env_indir"].max()) > 0 and float(one["etc/open"].max()) > 0


def test_lit_view_on_the_g16_model():
    from esr_nerf_amd.config import lts_cfg
    from esr_nerf_amd.esrnerf import ESRNeRF
    from esr_nerf_amd.sources import emissive_sources, extract_surface, simplify_surface
    from esr_nerf_amd.synthetic import slab_scene
    sc = slab_scene("g16", s_val=60.0, oblique=True, n_rays=1920, seed=0)
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = lts_cfg(DEV, num_2ndrays=8, num_ltspts=12)
    m = ESRNeRF(cfg, sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max, sc.mask_alpha_init,
                sc.mask_density, sc.s_val, sc.num_voxels)
    m.load_state_dict({k: torch.from_numpy(x).to(DEV) for k, x in load_npz("lts_g16_params.npz").items()})
    m.s_val = 60.0
    m.eval()
    surf = extract_surface(m, resolution=48)
    k_val = float(surf.attrs["emission"].max(dim=1).values.median())
    vv = surf.vertices
    h = 2.5 * float((vv.amax(0) - vv.amin(0)).max()) / 47.0
    small, _ = simplify_surface(surf, cell=h, face_source=emissive_sources(surf, k_val).face_source)
    rep = emissive_sources(small, k_val)
    v, tr = small.vertices.cpu().numpy(), small.triangles.cpu().numpy()
    attrs = {k: x.cpu().numpy() for k, x in small.attrs.items()}
    lo, hi = v.min(0), v.max(0)
    mid, ext = (lo + hi) / 2, float((hi - lo).max())
    cams, pose = _camera(mid + np.array([0.2, -0.3, 1.0]) * ext * 1.6, mid, [0.0, 1.0, 0.0], 22.0, 20, 16)
    sg = tuple(x.detach().cpu().numpy() for x in (m.envmap.mus, m.envmap.lambdas, m.envmap.lobes))
    one, two = _check_lit_view(small, rep, attrs, v, tr, cams, pose, sg, 64, "g16")
    # the model's own module is taken as it is
    from esr_nerf_amd import sources
    again = sources.lit_view(small, rep, cams, 0, samples=16, env=m.envmap, env_dirs=64)
    assert torch.equal(again["lin/env_dir"], one["lin/env_dir"]) and bool(torch.isfinite(two["lin/env_indir"]).all())
