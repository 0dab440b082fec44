"""The texture atlas on the host (CPU only): the footprint property of the layout's constants enumerated, the numpy restatement
tests/atlas_ref.py checked against brute force from the definitions, every mutant of atlas_ref.MUTANTS rejected by those
checks on each operation it applies to, header section W against the ctypes binding, and the writers of
sources.write_surface_obj read back."""
import os
import re
import struct
import zlib

import numpy as np
import pytest

import atlas_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


# ---------------------------------------------------------------- the footprint property

def sweep(l, g, leg_delta=0):
    """The points of half 0's triangle on the grid of quarter texels, as integers in quarter texels [n, 2]: corners and edges
    included.  A lookup's four texels depend on floor(p - 1/2) per axis alone, and a quarter-texel grid meets every combination
    of those classes that the triangle meets (the integers, the half-integer boundaries and the open intervals between them, on
    the hypotenuse as well, where x + y is an integer).  Up to 2^8 texels the whole grid; beyond, every point within three texels
    of an edge and a coarse grid of the interior, which is far from every texel another half owns."""
    e = 4 * (ar.leg(l, g) + leg_delta)
    if l <= 8:
        x, y = np.meshgrid(np.arange(e + 1), np.arange(e + 1), indexing="ij")
        keep = x + y <= e
        pts = np.stack([x[keep], y[keep]], 1)
    else:
        band, along = np.arange(13), np.arange(e + 1)
        a, b = np.meshgrid(band, along, indexing="ij")
        a, b = a.ravel(), b.ravel()
        parts = [np.stack([a, b], 1), np.stack([b, a], 1), np.stack([b, e - b - a], 1)]
        c = np.arange(0, e + 1, 61)
        cx, cy = np.meshgrid(c, c, indexing="ij")
        parts.append(np.stack([cx.ravel(), cy.ravel()], 1))
        pts = np.concatenate(parts)
        pts = pts[(pts >= 0).all(1) & (pts.sum(1) <= e)]
    return pts + 4 * g


def footprint_holds(l, g, mutant=None, leg_delta=0):
    s = 1 << l
    base = sweep(l, g, leg_delta)
    for half in (0, 1):
        p = base if half == 0 else 4 * s - base                        # the point reflection, in quarter texels
        i0, j0 = (p[:, 0] - 2) // 4, (p[:, 1] - 2) // 4                 # floor(p - 1/2)
        for di in (0, 1):
            for dj in (0, 1):
                i, j = i0 + di, j0 + dj
                owner = (i + j > s - 1 - (1 if mutant == "diagonal_to_wrong_half" else 0)).astype(np.int64)
                if not ((i >= 0) & (i < s) & (j >= 0) & (j < s) & (owner == half)).all():
                    return False
    return True


def test_sweep_is_the_triangle_of_the_restatement():
    for l, g in ((3, 1), (5, 2), (9, 1), (13, 3)):
        tri = ar.triangle(l, g, 0) * 4
        pts = sweep(l, g)
        for corner in tri:
            assert (pts == corner).all(1).any()
        assert (pts[:, 0] >= tri[0, 0]).all() and (pts[:, 1] >= tri[0, 1]).all() and (pts.sum(1) <= tri[1].sum()).all()
        assert (pts.sum(1) == tri[1].sum()).sum() >= ar.leg(l, g) * 4 + 1, "the whole hypotenuse"
        assert np.array_equal(ar.triangle(l, g, 1), (1 << l) - ar.triangle(l, g, 0))
        assert ar.owner(0, (1 << l) - 1, 1 << l) == 0 and ar.owner(1, (1 << l) - 1, 1 << l) == 1


@pytest.mark.parametrize("g", (1, 2, 3))
def test_footprint_property(g):
    for l in range(ar.low_level(g), 14):
        assert footprint_holds(l, g), (l, g)


def test_footprint_constants_are_tight():
    """With g = 1 one more texel of leg breaks the property, and so does the diagonal in the other half's hands.  (For a larger
    gutter the leg s - (3 g + 1) keeps g texels on either side of the diagonal; the property alone would allow g - 1 more.)"""
    for g in (1, 2, 3):
        for l in (ar.low_level(g) + 1, 9):
            assert footprint_holds(l, g, leg_delta=g - 1), (l, g)
            assert not footprint_holds(l, g, leg_delta=g), (l, g)
    assert not footprint_holds(4, 1, mutant="diagonal_to_wrong_half") and not footprint_holds(10, 1, mutant="diagonal_to_wrong_half")


# ---------------------------------------------------------------- the restatement against brute force

def cases():
    def make():
        out = {}
        cv, ct = ar.cube()
        for F in (0, 1, 2, 3):
            out[f"F={F}"] = (cv, ct[:F], 64, 1, 20.0, None, None)
        out["cube"] = (cv, ct, 64, 1, 9.0, None, None)
        out["cube g=2"] = (cv, ct, 128, 2, 14.0, None, None)
        sv_, st_ = ar.level_span(1, 3, 6)
        out["every level 3..6"] = (sv_, st_, 128, 1, 1.0, 3, 6)
        sv2, st2 = ar.level_span(2, 3, 5)
        out["every level 3..5 g=2"] = (sv2, st2, 64, 2, 1.0, 3, 5)
        out["odd faces"] = (*ar.odd_faces(), 64, 1, 6.0, None, 4)
        out["far faces"] = (*ar.far_faces(), 128, 1, 40.0, None, None)
        return out
    return memo("cases", make)


CASE_NAMES = ("F=0", "F=1", "F=2", "F=3", "cube", "cube g=2", "every level 3..6", "every level 3..5 g=2", "odd faces", "far faces")


def built(name, mutant=None):
    v, t, W, g, rho, lmin, lmax = cases()[name]
    return memo(("built", name, mutant), lambda: ar.build(v, t, W, g, rho, lmin, lmax, attr=ar.attributes(len(v)), mutant=mutant))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_against_brute_force(name):
    v, t, W, g, rho, lmin, lmax = cases()[name]
    a = built(name)
    assert a["fits"]
    ar.check_levels(v, t, a, rho)
    ar.check_layout(v, t, a)
    ar.check_texels(v, t, a)
    if name.startswith("every level"):
        used = np.nonzero(a["hist"])[0]
        assert list(used) == list(range(a["lmin"], a["lmax"] + 1)) and (a["hist"][used] % 2 == 1).sum() >= 2
    if name == "odd faces":
        assert a["level"][2] == a["lmin"] and a["level"][4] == a["lmin"] and a["level"][5] == a["lmin"]      # degenerate, NaN, overflow
        assert a["level"][8] == a["lmin"] and a["level"][9] == a["lmin"]                                      # bad vertex ids
        assert list(a["rot"][[0, 6, 7]]) == [0, 2, 1]                   # the same triangle from its three corners
        assert list(a["rot"][[10, 11, 12, 13]]) == [0, 0, 0, 1]         # equal longest edges: ties go to the smaller rot


def test_morton_decode_inverts_an_independent_interleave():
    rng = np.random.default_rng(0)
    x, y = rng.integers(0, 1 << 13, 500), rng.integers(0, 1 << 13, 500)
    u = np.array([ar.interleave(a, b) for a, b in zip(x, y)], np.int64)
    dx, dy = ar.morton_decode(u)
    assert np.array_equal(dx, x) and np.array_equal(dy, y)
    assert np.array_equal(ar.morton_encode(x, y), u)
    assert ar.interleave(1, 0) == 1 and ar.interleave(0, 1) == 2 and ar.interleave(3, 0) == 5


def test_fit_is_exact():
    v, t, W, g, rho, lmin, lmax = cases()["cube"]
    a = built("cube")
    _, _, _, used = ar.groups(a["hist"], a["lmin"], a["lmax"])
    assert used <= (W >> a["lmin"]) ** 2
    # 12 faces of level 5 (6 cells of 32 x 32) do not fit 64 x 64; 8 do
    h = np.zeros(ar.NL, np.int64)
    h[5] = 8
    assert ar.fits(h, 64, 3, 6)
    h[5] = 9
    assert not ar.fits(h, 64, 3, 6)
    h[5], h[3] = 6, 32                                                 # 3 cells of 16 units and 16 cells of one: the 64 units
    assert ar.fits(h, 64, 3, 6)
    h[3] = 33
    assert not ar.fits(h, 64, 3, 6)


def end_to_end_ratio(name, mutant=None):
    v, t, W, g, rho, lmin, lmax = cases()[name]
    a = built(name, mutant)
    attr = ar.attributes(len(v))
    qf, qb = ar.surface_queries(t, np.random.default_rng(1))
    got = ar.sample(a["uv"], W, a["tex"], qf, qb, mutant)
    return ar.end_to_end(v, t, built(name) if mutant in ("half_texel_dropped", "weights_wrong_axis") else a, attr, qf, qb, got)


@pytest.mark.parametrize("name", ("F=1", "F=3", "cube", "cube g=2", "every level 3..6", "every level 3..5 g=2", "far faces"))
def test_end_to_end_property_of_the_emulation(name):
    ratio = end_to_end_ratio(name)
    print(f"  {name:24s} worst ratio {ratio:.3f}")
    assert ratio <= ar.K
    assert ratio <= ar.WORST_EMULATION + 0.005


def rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# mutant -> (the case, the checks that must reject it: one per operation the mutant applies to)
def _levels(name, m):
    v, t, W, g, rho, *_ = cases()[name]
    ar.check_levels(v, t, built(name, m), rho)


def _layout(name, m):
    v, t, *_ = cases()[name]
    ar.check_layout(v, t, built(name, m))


def _texels(name, m):
    """the texel pass of the mutant on the charts of the true layout"""
    v, t, W, g, rho, lmin, lmax = cases()[name]
    a = dict(built(name))
    a.update(ar.texels(v, t, a["order"], a["rot"], a["hist"], W, g, a["lmin"], a["lmax"], ar.attributes(len(v)), mutant=m))
    ar.check_texels(v, t, a)


def _sample(name, m):
    assert end_to_end_ratio(name, m) <= ar.K


MUTANT_CHECKS = {
    "halves_swapped": ("cube", (_layout, _texels)),
    "diagonal_to_wrong_half": ("cube", (_texels,)),
    "rot_ignored": ("every level 3..6", (_layout, _texels)),
    "leg_off_by_one": ("every level 3..6", (_levels, _layout, _texels)),
    "ascending_levels": ("every level 3..6", (_layout,)),
    "unstable_ties": ("every level 3..6", (_layout,)),
    "morton_xy_swapped": ("every level 3..6", (_layout, _texels)),
    "clamped_barycentrics": ("cube", (_texels, _sample)),
    "odd_tail_mapped": ("every level 3..6", (_texels,)),
    "half_texel_dropped": ("cube", (_sample,)),
    "weights_wrong_axis": ("cube", (_sample,)),
}


@pytest.mark.parametrize("mutant", ar.MUTANTS)
def test_mutant_is_rejected(mutant):
    name, checks = MUTANT_CHECKS[mutant]
    for check in checks:
        check(name, None)                                               # the check passes on the restatement itself
        assert rejected(lambda: check(name, mutant)), (mutant, check.__name__)


def test_every_mutant_has_a_check():
    assert set(MUTANT_CHECKS) == set(ar.MUTANTS)


# ---------------------------------------------------------------- header and binding

def test_header_section_w_and_the_binding():
    import ctypes as C
    from esr_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    assert _lib.ABI_VERSION == int(re.search(r"#define ESR_ABI_VERSION (\d+)", header).group(1)) >= 46
    assert " * W. Texture atlas of the surface" in header
    p, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    want = {
        "esr_atlas_levels": [p, i64, p, i64, i32, i32, i32, i32, f64, p, p, p, p],
        "esr_atlas_charts": [i64, p, p, p, i32, i32, i32, i32, p, p, p],
        "esr_atlas_texels": [p, i64, p, i64, p, p, p, i32, i32, i32, i32, p, i32, p, p, p, p, p, p],
        "esr_atlas_sample": [p, i64, i32, p, i32, i64, p, p, p, p],
    }
    for name, args in want.items():
        assert _lib.SIGNATURES[name] == (C.c_int, args), name
    assert (_lib.ATLAS_MIN_SIZE, _lib.ATLAS_MAX_SIZE, _lib.ATLAS_MAX_LEVELS, _lib.ATLAS_MAX_CHANNELS) == (64, 8192, 16, 16)
    assert ar.NL == _lib.ATLAS_MAX_LEVELS
    src = open(os.path.join(ROOT, "esr_nerf_amd", "csrc", "atlas.hip")).read()
    for name in want:
        assert re.search(r"ESR_API int " + name + r"\(", src), name
    if os.path.exists(_lib.LIB_PATH):
        assert _lib.lib().esr_abi_version() == _lib.ABI_VERSION and all(hasattr(_lib.lib(), n) for n in want)


def test_python_layout_arguments():
    from esr_nerf_amd import atlas
    assert atlas._layout("t", 2048, 1, None, None) == (3, 11) and atlas._layout("t", 64, 2, None, None) == (3, 6)
    assert atlas._layout("t", 64, 3, None, None) == (4, 6)
    for g in range(1, 20):
        assert atlas._layout("t", 8192, g, None, None)[0] == ar.low_level(g)
    for bad in ((100, 1, None, None), (32, 1, None, None), (16384, 1, None, None), (64, 0, None, None), (64, 1, 2, None),
                (64, 1, None, 7), (64, 1, 5, 4), (64, True, None, None)):
        with pytest.raises(ValueError):
            atlas._layout("t", *bad)
    h = [0] * 16
    h[5] = 9
    assert not atlas.fits(h, 64, 3, 6) and atlas.leg(5, 1) == ar.leg(5, 1) == 28
    h[5] = 8
    assert atlas.fits(h, 64, 3, 6)


# ---------------------------------------------------------------- writers

def png_decode(data):
    """a small decoder of 8-bit non-interlaced PNGs: chunks, zlib, the five filters -> uint8 [H, W, C]"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, head = 8, b"", None
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xffffffff, "chunk CRC"
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        at += 12 + n
    w, h, depth, colour, comp, filt, lace = head
    assert depth == 8 and comp == 0 and filt == 0 and lace == 0 and colour in (0, 2)
    c = 3 if colour == 2 else 1
    raw = zlib.decompress(idat)
    stride = w * c
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int64)
    for y in range(h):
        ft, line = raw[y * (stride + 1)], np.frombuffer(raw, np.uint8, stride, y * (stride + 1) + 1).astype(np.int64)
        cur = np.zeros(stride, np.int64)
        for x in range(stride):
            left = cur[x - c] if x >= c else 0
            up, ul = prev[x], (prev[x - c] if x >= c else 0)
            if ft == 0:
                pred = 0
            elif ft == 1:
                pred = left
            elif ft == 2:
                pred = up
            elif ft == 3:
                pred = (left + up) // 2
            else:
                pa, pb, pc = abs(up - ul), abs(left - ul), abs(left + up - 2 * ul)
                pred = left if pa <= pb and pa <= pc else up if pb <= pc else ul
            cur[x] = (line[x] + pred) & 255
        out[y], prev = cur, cur
    return out.reshape(h, w, c)


def hdr_decode(data):
    """a flat (non-RLE) Radiance picture -> float32 [H, W, 3]"""
    head, _, rest = data.partition(b"\n\n")
    assert head.startswith(b"#?RADIANCE") and b"FORMAT=32-bit_rle_rgbe" in head
    size, _, body = rest.partition(b"\n")
    m = re.fullmatch(rb"-Y (\d+) \+X (\d+)", size)
    h, w = int(m.group(1)), int(m.group(2))
    px = np.frombuffer(body, np.uint8).reshape(h, w, 4).astype(np.float64)
    scale = np.where(px[..., 3:] > 0, np.ldexp(1.0, px[..., 3:].astype(np.int64) - 136), 0.0)
    return (px[..., :3] * scale).astype(np.float32)


def test_png_round_trip(tmp_path):
    from esr_nerf_amd import sources
    rng = np.random.default_rng(0)
    for shape in ((5, 7, 3), (4, 4), (1, 1, 3), (9, 3, 1)):
        img = rng.integers(0, 256, shape).astype(np.uint8)
        data = sources.png_bytes(img)
        assert np.array_equal(png_decode(data), img.reshape(shape[0], shape[1], -1))
    # quantisation: clamped to [0, 1], rounded half to even
    x = np.array([[-1.0, 0.0, 0.2, 0.999, 1.0, 7.0, np.nan, 0.5 / 255, 1.5 / 255, 2.5 / 255]])
    halves = [int(np.rint(q * 255.0)) for q in x[0, 7:]]                # (where the binary64 product is a tie, it goes to even)
    assert list(sources.quantise8(x)[0]) == [0, 0, 51, 255, 255, 255, 0] + halves and all(h in (0, 1, 2, 3) for h in halves)


def test_hdr_round_trip():
    from esr_nerf_amd import sources
    rng = np.random.default_rng(1)
    img = (rng.random((6, 5, 3)) * np.array([1e-3, 1.0, 40.0])).astype(np.float32)
    img[0, 0] = 0.0
    back = hdr_decode(sources.hdr_bytes(img))
    top = img.max(-1, keepdims=True)
    step = np.where(top > 0, np.ldexp(1.0, np.frexp(top)[1] - 8), 0.0)      # one RGBE step of the pixel's exponent
    assert (np.abs(back - img) <= step).all() and (back[0, 0] == 0).all()


def test_obj_and_mtl_parse_back(tmp_path):
    import torch
    from esr_nerf_amd import sources
    from esr_nerf_amd.atlas import Atlas
    v, t, W, g, rho, lmin, lmax = cases()["cube"]
    a = built("cube")
    dev = "cpu"
    atlas = Atlas(W, g, a["lmin"], a["lmax"], rho, tuple(int(x) for x in a["hist"]), torch.from_numpy(a["level"]), torch.from_numpy(a["rot"]),
                  torch.from_numpy(a["order"]), torch.from_numpy(a["chart"]), torch.from_numpy(a["uv"]), torch.from_numpy(a["face"]),
                  torch.from_numpy(a["bary"]), torch.from_numpy(a["point"]), torch.from_numpy(a["flags"]))
    surface = sources.Surface(torch.from_numpy(v), torch.from_numpy(t), {})
    rng = np.random.default_rng(2)
    tex = {"basecolor": rng.random((W, W, 3)), "roughness": rng.random((W, W)), "metallic": rng.random((W, W)),
           "emission": rng.random((W, W, 3)) * 5, "normal": rng.normal(size=(W, W, 3))}
    tex = {k: torch.from_numpy(x.astype(np.float32)) for k, x in tex.items()}
    path = str(tmp_path / "mesh.obj")
    files = sources.write_surface_obj(path, surface, atlas, tex, gamma=lambda x: x ** (1 / 2.2))     # (the curve itself is a device kernel)
    lines = open(path).read().splitlines()
    assert "mtllib mesh.mtl" in lines
    pv = np.array([[float(x) for x in l.split()[1:]] for l in lines if l.startswith("v ")])
    pvt = np.array([[float(x) for x in l.split()[1:]] for l in lines if l.startswith("vt ")])
    pf = np.array([[[int(x) for x in c.split("/")] for c in l.split()[1:]] for l in lines if l.startswith("f ")])
    assert np.array_equal(pv, v), "v round-trips (repr of the doubles)"
    assert np.array_equal(pf[:, :, 0] - 1, t)
    assert np.array_equal(pf[:, :, 1] - 1, np.arange(3 * len(t)).reshape(-1, 3))
    uv = a["uv"].reshape(-1, 2).astype(np.float64)
    assert np.array_equal(pvt, np.stack([uv[:, 0], 1.0 - uv[:, 1]], 1)), "vt.v = 1 - y / W, exactly"
    mtl = dict(l.split(None, 1) for l in open(str(tmp_path / "mesh.mtl")).read().splitlines() if l and not l.startswith("#"))
    for key in ("map_Kd", "map_Pr", "map_Pm", "map_Ke", "norm"):
        assert os.path.exists(str(tmp_path / mtl[key])), key
    assert set(os.path.basename(f) for f in files) >= {"mesh.obj", "mesh.mtl", "mesh_emission.hdr", "mesh_emission.npy"}
    rough = png_decode(open(str(tmp_path / mtl["map_Pr"]), "rb").read())[..., 0]
    assert np.array_equal(rough, sources.quantise8(tex["roughness"].numpy().astype(np.float64)))
    base = png_decode(open(str(tmp_path / mtl["map_Kd"]), "rb").read())
    assert np.array_equal(base, sources.quantise8((tex["basecolor"] ** (1 / 2.2)).numpy().astype(np.float64)))
    assert np.array_equal(np.load(str(tmp_path / "mesh_emission.npy")), tex["emission"].numpy())
    em = hdr_decode(open(str(tmp_path / "mesh_emission.hdr"), "rb").read())
    assert np.abs(em - tex["emission"].numpy()).max() <= 5 * 2.0 ** -7
