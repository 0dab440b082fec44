"""Section W on the device (esr_atlas_levels / charts / texels / sample through the C ABI, and atlas.py / sources.py above them)
against tests/atlas_ref.py.

Integers (levels, rot, histogram, charts, faces, flags) and the binary64 results (uv, bary, point) equal the restatement
exactly; the interpolated texture and the sampler are bit-equal to the binary32 emulation.  Every output sits between guard
bytes at a pointer that is 8- but not 32-byte aligned, one case runs on inputs that start one row into their allocation, a
refused call leaves its outputs at their prefill and two runs give the same bytes.  The end-to-end property -- bake the vertex
attributes, look them up again, get the barycentric interpolation within K 2^-24 absref -- holds at every point; the worst
ratios are printed (-s): the constants of atlas_ref.py come from them."""
import ctypes

import numpy as np
import pytest
import torch

import atlas_ref as ar
from conftest import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, FILL = 64, 0xA5
_memo = {}
WORST = {"emulation": 0.0, "device": 0.0}


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


def untouched(x):
    return bool((x.reshape(-1).view(torch.uint8) == FILL).all())


def shifted(x):
    """a device copy of x that starts one row into its allocation"""
    x = torch.from_numpy(np.ascontiguousarray(x))
    buf = torch.zeros((x.shape[0] + 1,) + tuple(x.shape[1:]), dtype=x.dtype, device=DEV)
    buf[1:] = x.to(DEV)
    return buf[1:]


def mc_sphere():
    """the marching-cubes sphere of test_gpu_simplify.py: a 24^3 field, 3 216 faces, in a box of side 2"""
    def build():
        from esr_nerf_amd import mesh
        ax = torch.arange(24, dtype=torch.float32, device=DEV)
        x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
        u = 9.3 - torch.sqrt((x - 11.3) ** 2 + (y - 11.6) ** 2 + (z - 11.45) ** 2)
        v, t = mesh.marching_cubes(u.contiguous())
        v, t = v.cpu().numpy() * (2.0 / 23.0) - 1.0, t.cpu().numpy()
        assert len(t) == 3216 and v.dtype == np.float64
        return v, t
    return memo("mc_sphere", build)


def cases():
    """name -> (v, t, W, g, rho, lmin, lmax, channels)"""
    def make():
        out = {}
        cv, ct = ar.cube()
        for F in (0, 1, 2, 3):
            out[f"F={F}"] = (cv, ct[:F], 64, 1, 20.0, None, None, 12)
        out["cube W=64"] = (cv, ct, 64, 1, 9.0, None, None, 12)
        out["cube W=128 g=2"] = (cv, ct, 128, 2, 14.0, None, None, 12)
        out["every level 3..6"] = (*ar.level_span(1, 3, 6), 128, 1, 1.0, 3, 6, 12)
        out["every level 3..5 g=2"] = (*ar.level_span(2, 3, 5), 64, 2, 1.0, 3, 5, 16)
        out["odd faces"] = (*ar.odd_faces(), 64, 1, 6.0, None, 4, 3)
        out["far faces"] = (*ar.far_faces(), 128, 1, 40.0, None, None, 12)
        # the sphere at the first density of a fixed ladder whose layout fits (found on the restatement's level pass)
        sv, st = mc_sphere()
        rho = next(r for r in (200.0 * 0.95 ** k for k in range(200)) if ar.fits(ar.levels(sv, st, 1, 3, 9, r ** 4)[2], 512, 3, 9))
        out["mc sphere W=512"] = (sv, st, 512, 1, rho, None, None, 12)
        out["cube W=2048"] = (cv, ct, 2048, 1, 300.0, None, None, 1)         # the texel pass strides: four trips of its grid
        return out
    return memo("cases", make)


CASE_NAMES = ("F=0", "F=1", "F=2", "F=3", "cube W=64", "cube W=128 g=2", "every level 3..6", "every level 3..5 g=2", "odd faces",
              "far faces", "mc sphere W=512", "cube W=2048")


def reference(name):
    v, t, W, g, rho, lmin, lmax, C = cases()[name]
    return memo(("ref", name), lambda: ar.build(v, t, W, g, rho, lmin, lmax, attr=ar.attributes(len(v), C)))


def run_chain(name, shift=False, counts=None, lmax_over=None):
    """the four entries through the C ABI with guarded outputs -> dict of numpy arrays and the codes.  `counts`: a level table
    that replaces the histogram at the charts and texels entries"""
    from esr_nerf_amd import _lib
    L = _lib.lib()
    v, t, W, g, rho, lmin, lmax, C = cases()[name]
    ref = reference(name)
    lmin, lmax = ref["lmin"], ref["lmax"] if lmax_over is None else lmax_over
    up = shifted if shift else dev
    F, V = len(t), len(v)
    attr = ar.attributes(V, C)
    d = dict(v=up(v), t=up(t), attr=up(attr))
    before = {k: x.clone() for k, x in d.items()}
    st = _lib.stream_ptr(DEV)
    rho2 = float(rho) * float(rho)
    out = {}
    raws = {}

    def g_out(key, shape, dtype):
        raws[key] = guarded(shape, dtype)
        return raws[key][1]
    level, rot, hist = g_out("level", (F,), torch.int32), g_out("rot", (F,), torch.int32), g_out("hist", (16,), torch.int64)
    out["code_levels"] = L.esr_atlas_levels(_lib.ptr(d["v"]), V, _lib.ptr(d["t"]), F, W, g, lmin, lmax, rho2 * rho2, _lib.ptr(level),
                                            _lib.ptr(rot), _lib.ptr(hist), st)
    torch.cuda.synchronize()
    assert out["code_levels"] == 0
    host = hist.cpu().numpy() if counts is None else np.asarray(counts, np.int64)
    order = torch.sort(lmax - level, stable=True).indices.contiguous()
    table = (ctypes.c_int64 * 16)(*[int(x) for x in host])
    chart, uv = g_out("chart", (F, 4), torch.int32), g_out("uv", (F, 3, 2), torch.float32)
    out["code_charts"] = L.esr_atlas_charts(F, _lib.ptr(order), _lib.ptr(rot), table, W, g, lmin, lmax, _lib.ptr(chart), _lib.ptr(uv), st)
    face, bary, point = g_out("face", (W, W), torch.int32), g_out("bary", (W, W, 2), torch.float32), g_out("point", (W, W, 3), torch.float32)
    flags, tex = g_out("flags", (W, W), torch.uint8), g_out("tex", (W, W, C), torch.float32)
    out["code_texels"] = L.esr_atlas_texels(_lib.ptr(d["v"]), V, _lib.ptr(d["t"]), F, _lib.ptr(order), _lib.ptr(rot), table, W, g, lmin, lmax,
                                            _lib.ptr(d["attr"]), C, _lib.ptr(face), _lib.ptr(bary), _lib.ptr(point), _lib.ptr(flags),
                                            _lib.ptr(tex), st)
    torch.cuda.synchronize()
    for key, (raw, x, n) in raws.items():
        assert guards_intact(raw, n), (key, "a guard byte was written")
    for k, x in d.items():
        assert not x.numel() or torch.equal(x.view(torch.uint8), before[k].view(torch.uint8)), (k, "an input changed")
    if out["code_charts"] != 0:
        assert untouched(chart) and untouched(uv), "written by a refused call"
    if out["code_texels"] != 0:
        assert all(untouched(x) for x in (face, bary, point, flags, tex)), "written by a refused call"
    out.update(level=level, rot=rot, hist=hist, order=order, chart=chart, uv=uv, face=face, bary=bary, point=point, flags=flags, tex=tex)
    return {k: (x.cpu().numpy() if isinstance(x, torch.Tensor) else x) for k, x in out.items()}, dict(uv=uv, tex=tex)


def bits(x):
    """the bit patterns of a float32 array, every NaN as one pattern (the sign of a generated NaN is the machine's)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return np.where(np.isnan(x), np.uint32(0x7fc00000), x.view(np.uint32))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_chain_equals_the_restatement(name):
    v, t, W, g, rho, lmin, lmax, C = cases()[name]
    ref = reference(name)
    assert ref["fits"]
    got, _ = run_chain(name, shift=name == "every level 3..6")
    assert got["code_charts"] == 0 and got["code_texels"] == 0
    for key in ("level", "rot", "hist", "order", "chart", "face", "flags"):
        assert np.array_equal(got[key], ref[key]), key
    for key in ("uv", "bary", "point", "tex"):
        assert np.array_equal(bits(got[key]), bits(ref[key])), (key, "bit for bit")
    # every owned texel lies in the half of its face's cell, and as many texels are owned as the restatement says
    a = dict(ref)
    a.update({k: got[k] for k in ("chart", "uv", "face", "bary", "point", "flags", "level", "rot", "order")})
    assert np.array_equal(got["face"], ar.brute_texel_owner(a))
    assert int((got["face"] >= 0).sum()) == int((ref["face"] >= 0).sum())
    if W <= 512:
        ar.check_layout(v, t, a)
        ar.check_texels(v, t, a)
    again, _ = run_chain(name)
    for key in ("level", "rot", "hist", "chart", "uv", "face", "bary", "point", "flags", "tex"):
        assert got[key].tobytes() == again[key].tobytes(), (key, "two runs")
    print(f"  {name:24s} {len(t)} faces, levels {dict((l, int(n)) for l, n in enumerate(ref['hist']) if n)}, "
          f"{float((got['face'] >= 0).mean()):.3f} of the texels owned, {float((got['flags'] & 1).mean()):.3f} inside")


def test_an_atlas_one_cell_too_small_is_refused():
    """9 faces of level 5 need five cells of 32 x 32; 64 x 64 holds four"""
    from esr_nerf_amd import _lib, atlas
    cv, ct = ar.cube()
    cases()["nine large"] = (cv, ct[:9], 64, 1, 1000.0, None, 5, 3)
    ref = reference("nine large")
    assert list(ref["hist"][[5]]) == [9] and not ref["fits"]
    got, _ = run_chain("nine large")
    assert got["code_charts"] == _lib.ECAP and got["code_texels"] == _lib.ECAP
    cases()["eight large"] = (cv, ct[:8], 64, 1, 1000.0, None, 5, 3)
    got, _ = run_chain("eight large")
    assert got["code_charts"] == 0 and got["code_texels"] == 0 and (got["face"] >= 0).all(), "four cells, eight halves: every texel owned"
    # counts that are not the faces': refused as bad arguments, nothing written
    bad = np.zeros(16, np.int64)
    bad[5] = 7
    got, _ = run_chain("eight large", counts=bad)
    assert got["code_charts"] == _lib.EINVAL and got["code_texels"] == _lib.EINVAL
    with pytest.raises(ValueError):
        atlas.build(dev(cv), dev(ct[:9]), size=64, texels_per_unit=1000.0, lmax=5)


def test_bad_arguments_are_refused():
    from esr_nerf_amd import _lib
    L = _lib.lib()
    st = _lib.stream_ptr(DEV)
    cv, ct = ar.cube()
    v, t = dev(cv), dev(ct)
    level, rot = torch.zeros(12, dtype=torch.int32, device=DEV), torch.zeros(12, dtype=torch.int32, device=DEV)
    hist = torch.zeros(16, dtype=torch.int64, device=DEV)
    base = dict(size=64, g=1, lmin=3, lmax=6, rho4=1.0)
    for over, want in ((dict(size=96), _lib.EINVAL), (dict(size=32), _lib.EINVAL), (dict(size=16384), _lib.EINVAL), (dict(g=0), _lib.EINVAL),
                       (dict(lmin=2), _lib.EINVAL), (dict(lmax=7), _lib.EINVAL), (dict(lmin=5, lmax=4), _lib.EINVAL),
                       (dict(rho4=float("nan")), _lib.EINVAL), (dict(rho4=-1.0), _lib.EINVAL), (dict(rho4=float("inf")), _lib.EINVAL)):
        a = {**base, **over}
        code = L.esr_atlas_levels(_lib.ptr(v), 8, _lib.ptr(t), 12, a["size"], a["g"], a["lmin"], a["lmax"], a["rho4"], _lib.ptr(level),
                                  _lib.ptr(rot), _lib.ptr(hist), st)
        assert code == want, over
    assert L.esr_atlas_levels(_lib.ptr(v), 8, _lib.ptr(t), 12, 64, 1, 3, 6, 1.0, _lib.ptr(level), ctypes.c_void_p(rot.data_ptr() + 2),
                              _lib.ptr(hist), st) == _lib.EINVAL
    assert L.esr_atlas_levels(_lib.ptr(v), 8, _lib.ptr(t), 1 << 31, 64, 1, 3, 6, 1.0, _lib.ptr(level), _lib.ptr(rot), _lib.ptr(hist), st) == _lib.ECAP
    out = torch.zeros(4, 17, dtype=torch.float32, device=DEV)
    tex = torch.zeros(64, 64, 17, dtype=torch.float32, device=DEV)
    uv = torch.zeros(12, 3, 2, dtype=torch.float32, device=DEV)
    qf, qb = torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(4, 2, dtype=torch.float64, device=DEV)
    assert L.esr_atlas_sample(_lib.ptr(uv), 12, 64, _lib.ptr(tex), 17, 4, _lib.ptr(qf), _lib.ptr(qb), _lib.ptr(out), st) == _lib.ECAP
    assert L.esr_atlas_sample(_lib.ptr(uv), 12, 64, _lib.ptr(tex), 0, 4, _lib.ptr(qf), _lib.ptr(qb), _lib.ptr(out), st) == _lib.EINVAL
    assert L.esr_atlas_sample(_lib.ptr(uv), 12, 64, None, 3, 4, _lib.ptr(qf), _lib.ptr(qb), _lib.ptr(out), st) == _lib.EINVAL
    assert L.esr_atlas_sample(None, 12, 64, None, 3, 0, None, None, None, st) == 0
    torch.cuda.synchronize()


def sample_abi(uv, tex, W, qf, qb):
    """one guarded call of esr_atlas_sample on device uv / tex"""
    from esr_nerf_amd import _lib
    n, C = len(qf), int(tex.shape[2])
    raw, out, nb = guarded((n, C), torch.float32)
    f, b = dev(qf.astype(np.int32)), dev(np.asarray(qb, np.float64))
    code = _lib.lib().esr_atlas_sample(_lib.ptr(uv), int(uv.shape[0]), W, _lib.ptr(tex), C, n, _lib.ptr(f), _lib.ptr(b), _lib.ptr(out),
                                       _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert code == 0 and guards_intact(raw, nb)
    return out.cpu().numpy()


@pytest.mark.parametrize("name", ("F=1", "F=3", "cube W=64", "cube W=128 g=2", "every level 3..6", "every level 3..5 g=2", "far faces",
                                  "mc sphere W=512"))
def test_bake_and_lookup_reproduce_the_interpolation(name):
    v, t, W, g, rho, lmin, lmax, C = cases()[name]
    ref = reference(name)
    got, on_dev = run_chain(name)
    attr = ar.attributes(len(v), C)
    qf, qb = ar.surface_queries(t, np.random.default_rng(1))
    # stray queries: no face, a face id past the end, barycentrics that are not finite or far outside
    stray_f = np.array([-1, len(t), 0, 0, 0], np.int32)
    stray_b = np.array([[0.2, 0.2], [0.2, 0.2], [np.nan, 0.1], [np.inf, 0.0], [-40.0, 90.0]])
    out = sample_abi(on_dev["uv"].contiguous(), on_dev["tex"].contiguous(), W, np.concatenate([qf, stray_f]), np.concatenate([qb, stray_b]))
    emu = ar.sample(ref["uv"], W, ref["tex"], np.concatenate([qf, stray_f]), np.concatenate([qb, stray_b]))
    assert np.array_equal(bits(out), bits(emu)), "the sampler, bit for bit"
    assert (out[len(qf):len(qf) + 4] == 0).all()
    a = dict(ref)
    a.update({k: got[k] for k in ("chart", "uv", "face", "bary", "point", "flags")})
    r_dev = ar.end_to_end(v, t, a, attr, qf, qb, out[:len(qf)])
    r_emu = ar.end_to_end(v, t, ref, attr, qf, qb, emu[:len(qf)])
    WORST["device"], WORST["emulation"] = max(WORST["device"], r_dev), max(WORST["emulation"], r_emu)
    print(f"  {name:24s} worst ratio {r_dev:.3f} (the emulation's {r_emu:.3f}) over {len(qf)} points x {C} channels; so far {WORST}")
    assert r_dev <= ar.K and r_emu <= ar.K
    assert r_dev <= ar.WORST_MI355X + 0.005 and r_emu <= ar.WORST_EMULATION + 0.005, "the recorded worst ratios are the worst"


def test_python_build_and_density_search():
    from esr_nerf_amd import atlas
    v, t = mc_sphere()
    dv, dt = dev(v), dev(t)
    a = atlas.build(dv, dt, size=512)
    assert atlas.fits(a.counts, 512, a.lmin, a.lmax) and sum(a.counts) == len(t) and (a.lmin, a.lmax, a.gutter) == (3, 9, 1)
    # the density found is the restatement's layout at that density, and a little more no longer fits
    ref = ar.build(v, t, 512, 1, a.density)
    for key in ("level", "rot", "order", "chart", "face", "flags"):
        assert np.array_equal(getattr(a, key).cpu().numpy(), ref[key]), key
    for key in ("uv", "bary", "point"):
        assert np.array_equal(bits(getattr(a, key).cpu().numpy()), bits(ref[key])), key
    assert tuple(a.counts) == tuple(int(x) for x in ref["hist"])
    more = ar.build(v, t, 512, 1, a.density * 1.01)
    assert not more["fits"], "1 % more density still fits: the search stopped early"
    b = atlas.build(dv, dt, size=512, texels_per_unit=a.density)
    assert torch.equal(b.chart, a.chart) and torch.equal(b.face, a.face) and torch.equal(b.point.view(torch.int32), a.point.view(torch.int32))
    fill = float((a.face >= 0).float().mean())
    print(f"  mc sphere in 512 x 512: density {a.density:.2f} texels per unit, counts {dict((l, n) for l, n in enumerate(a.counts) if n)}, "
          f"{fill:.3f} owned, {float((a.flags & 1).float().mean()):.3f} inside")
    assert fill > 0.25
    # sample: the wrapper is the entry
    attr = dev(ar.attributes(len(v), 12))
    tex = atlas.texels(a, dv, dt, attr)[4]
    qf, qb = ar.surface_queries(t[:50], np.random.default_rng(2), 8)
    got = atlas.sample(a, tex, dev(qf), dev(qb)).cpu().numpy()
    assert np.array_equal(bits(got), bits(ar.sample(ref["uv"], 512, tex.cpu().numpy(), qf, qb)))
    one = atlas.sample(a, tex[:, :, 3].contiguous(), dev(qf), dev(qb).float())
    assert one.shape == (len(qf),)
    empty = atlas.build(dv, dt[:0], size=64)
    assert int((empty.face >= 0).sum()) == 0 and empty.uv.shape == (0, 3, 2)
    for bad in (dict(size=100), dict(gutter=0), dict(lmin=2), dict(texels_per_unit=float("nan"))):
        with pytest.raises(ValueError):
            atlas.build(dv, dt, **{"size": 512, **bad})


# ---------------------------------------------------------------- the model bake

def g16():
    def build():
        from esr_nerf_amd.config import lts_cfg
        from esr_nerf_amd.esrnerf import ESRNeRF
        from esr_nerf_amd.sources import emissive_sources, extract_surface, simplify_surface
        from esr_nerf_amd.synthetic import slab_scene
        from esr_nerf_amd import atlas, raycast
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
        assert len(rep) >= 1
        at = atlas.build(small.vertices, small.triangles, size=256)
        return m, small, rep, k_val, at, raycast.build(small.vertices, small.triangles)
    return memo("g16", build)


def g16_camera(small):
    from esr_nerf_amd.camera import Cameras
    v = small.vertices.cpu().numpy()
    lo, hi = v.min(0), v.max(0)
    mid, ext = (lo + hi) / 2, float((hi - lo).max())
    eye = mid + np.array([0.2, -0.3, 1.0]) * ext * 1.6
    fwd = (mid - eye) / np.linalg.norm(mid - eye)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    pose = np.stack([right, np.cross(fwd, right), fwd, eye], 1).astype(np.float32)
    return Cameras(torch.from_numpy(pose[None]).to(DEV), 22.0, 22.0, 10.0, 8.0, 20, 16)


def test_model_bake_is_the_model_at_the_texels():
    from esr_nerf_amd import mesh, sources
    m, small, rep, k_val, at, bvh = g16()
    tex = sources.bake_materials(small, at, model=m)
    own = at.face >= 0
    assert int(own.sum()) > 1000 and set(tex) == set(sources.ATTR_KEYS)
    lo, hi = (b.to(DEV) for b in mesh._box(m))
    pts = torch.minimum(torch.maximum(at.point[own], lo), hi)
    direct = m.surface_attributes(pts, chunk=1 << 12)                     # (another chunking: the values are per point)
    for k in sources.ATTR_KEYS:
        assert tex[k].shape[:2] == (256, 256)
        assert torch.equal(tex[k][own].reshape(-1).view(torch.int32), direct[k].float().reshape(-1).view(torch.int32)), (k, "bit for bit")
        assert float(tex[k][~own].abs().max()) == 0.0 if bool((~own).any()) else True
    # emissive texels: inside the faces of a source, the share above k_val is the share the model gives at the same points
    in_src = own & ((at.flags & 1) != 0) & (rep.face_source[at.face.clamp(min=0).long()] >= 0)
    assert int(in_src.sum()) > 0
    share = float((tex["emission"][in_src].max(dim=1).values > k_val).float().mean())
    sel = in_src[own]
    want = float((direct["emission"][sel].max(dim=1).values > k_val).float().mean())
    print(f"  g16: {small.triangles.shape[0]} faces, density {at.density:.1f}, {int(own.sum())} texels owned, {int(in_src.sum())} inside "
          f"source faces, {share:.3f} of them above k_val")
    assert share == want and share > 0.5
    # without a model: the texel pass's own interpolation, key by key
    flat = sources.bake_materials(small, at)
    packed = torch.cat([small.attrs[k].reshape(small.vertices.shape[0], -1).float() for k in sources.ATTR_KEYS], dim=1).contiguous()
    ref = ar.texels(small.vertices.cpu().numpy(), small.triangles.cpu().numpy(), at.order.cpu().numpy(), at.rot.cpu().numpy(),
                    np.array(at.counts), 256, 1, at.lmin, at.lmax, packed.cpu().numpy())
    assert np.array_equal(bits(flat["basecolor"].cpu().numpy()), bits(ref["tex"][:, :, 4:7]))
    assert np.array_equal(bits(flat["metallic"].cpu().numpy()), bits(ref["tex"][:, :, 8]))
    assert np.array_equal(bits(at.point.cpu().numpy()), bits(ref["point"])) and np.array_equal(at.face.cpu().numpy(), ref["face"])


def parent_lit_view(surface, report, cams, view, samples, bvh):
    """lit_view as it was before the atlas keywords, from its public parts"""
    from esr_nerf_amd import raycast, sources
    H, W = cams.height, cams.width
    o, d, _ = raycast.pixel_rays(cams, view)
    hit = raycast.cast(bvh, o, d)
    got = hit.face >= 0
    x, normal, a, wo = sources._hit_points(surface, hit, d)
    lights = sources.source_lights(surface, report, samples, None)
    reflect = sources.direct_light(surface, lights, x, normal, a["basecolor"], a["roughness"][:, 0], a["metallic"][:, 0], wo, bvh=bvh)
    src = report.face_source[hit.face.clamp(min=0).long()]
    zero = torch.zeros(1, 3, dtype=torch.float32, device=x.device)
    return {"lin/reflect": torch.where(got[:, None], reflect, zero).reshape(H, W, 3),
            "lin/emit": torch.where((got & (src >= 0))[:, None], a["emission"].contiguous(), zero).reshape(H, W, 3),
            "face": hit.face.reshape(H, W), "depth": hit.t.reshape(H, W)}


def test_lit_view_from_textures():
    from esr_nerf_amd import sources
    m, small, rep, k_val, at, bvh = g16()
    cams = g16_camera(small)
    plain = sources.lit_view(small, rep, cams, 0, samples=16, bvh=bvh)
    parent = parent_lit_view(small, rep, cams, 0, 16, bvh)
    assert list(plain) == list(parent) == ["lin/reflect", "lin/emit", "face", "depth"]
    for k in parent:
        assert plain[k].dtype == parent[k].dtype and plain[k].cpu().numpy().tobytes() == parent[k].cpu().numpy().tobytes(), k
    env = tuple(torch.from_numpy(x).to(DEV) for x in (np.random.default_rng(3).random((4, 3)).astype(np.float32),
                                                       np.full(4, 3.0, np.float32), np.random.default_rng(4).normal(size=(4, 3)).astype(np.float32)))
    tex = sources.bake_materials(small, at, model=m)
    img = sources.lit_view(small, rep, cams, 0, samples=16, bvh=bvh, env=env, env_dirs=16, atlas=at, textures=tex)
    assert torch.equal(img["face"], plain["face"]) and torch.equal(img["depth"], plain["depth"])
    assert set(img) == {"lin/reflect", "lin/emit", "face", "depth", "lin/env_dir", "etc/open"}
    for k in ("lin/reflect", "lin/emit", "lin/env_dir"):
        assert bool(torch.isfinite(img[k]).all()), k
    hit = plain["face"] >= 0
    assert int(hit.sum()) > 20 and float(img["lin/reflect"][hit].abs().sum()) > 0 and float(img["lin/reflect"][~hit].abs().sum()) == 0
    # with the vertex attributes baked, the texture path is the vertex path up to the lookups' rounding
    flat = sources.bake_materials(small, at)
    same = sources.lit_view(small, rep, cams, 0, samples=16, bvh=bvh, atlas=at, textures=flat)
    scale = float(plain["lin/reflect"].abs().max())
    assert float((same["lin/reflect"] - plain["lin/reflect"]).abs().max()) <= 1e-3 * scale
    with pytest.raises(ValueError):
        sources.lit_view(small, rep, cams, 0, atlas=at)


def test_irradiance_bake_is_the_light_at_the_texels():
    from esr_nerf_amd import sources
    m, small, rep, k_val, at, bvh = g16()
    rng = np.random.default_rng(5)
    env = tuple(torch.from_numpy(x).to(DEV) for x in (rng.random((3, 3)).astype(np.float32), np.full(3, 2.0, np.float32),
                                                       rng.normal(size=(3, 3)).astype(np.float32)))
    edits = [dict(sources=[0], mode="i_change", intensity=2.0)]
    out = sources.bake_irradiance(small, at, rep, samples=8, edits=edits, env=env, env_dirs=16, bvh=bvh, chunk=5000)
    S = len(rep)
    assert out["light/sources"].shape == (256, 256, S, 3) and out["light/env"].shape == (256, 256, 3)
    inside = (at.flags & 1) != 0
    face = at.face[inside].contiguous()
    pts, nrm = at.point[inside].double(), sources.face_normals(small)[face.long()]
    lights = sources.source_lights(small, rep, 8, edits)
    want = sources.direct_light(small, lights, pts, nrm, bvh=bvh, per_source=True)
    assert torch.equal(out["light/sources"][inside].view(torch.int32), want.view(torch.int32))
    want_env = sources.environment_light(small, env, pts, nrm, dirs=16, faces=face, bvh=bvh)
    assert torch.equal(out["light/env"][inside].view(torch.int32), want_env.view(torch.int32))
    assert float(out["light/sources"][~inside].abs().max()) == 0.0 and float(out["light/env"][~inside].abs().max()) == 0.0
    assert float(out["light/sources"].max()) > 0 and float(out["light/env"].max()) > 0
    assert "light/env" not in sources.bake_irradiance(small, at, rep, samples=8, bvh=bvh)
