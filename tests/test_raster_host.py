"""The rasteriser's restatement checked without a GPU (tests/raster_ref.py: ray casting) against a SECOND restatement, the
definition of csrc/raster.hip in float64 numpy (projection, edge functions, 1 / sum(b / z)); a binary32-keyed emulation of
the z-buffer word for the tie rule; mutants of the definition, each of which the ray cast rejects; the C header against
the ctypes signatures; and what raster.py refuses before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import raster_ref as rr
from conftest import ROOT

Z_NEAR = 1e-6
ENTRIES = ("esr_raster_faces", "esr_raster_resolve", "esr_source_masks")
CAP = 0.005                                   # most ambiguous pixels the restatement may set aside on a generic case
_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def w2c_of(cam, view):
    m = np.eye(4)
    m[:3] = cam.poses[view].astype(np.float64)
    return np.linalg.inv(m)[:3]


def project_view(vertices, triangles, cam, view, z_near, mutant=None, key32=False):
    """the definition, vectorised over [pixel, face]; ``mutant`` breaks one rule; ``key32`` picks the winner by the
    (binary32 depth bits, face id) word instead of the float64 depth"""
    v, tr = np.asarray(vertices, np.float64), np.asarray(triangles, np.int64).reshape(-1, 3)
    W = w2c_of(cam, view)
    P = cam.width * cam.height
    with np.errstate(all="ignore"):
        pc = v @ W[:, :3].T + W[:, 3]
        zc = pc[:, 2]
        if mutant == "centroid_drop":
            dropped = zc[tr].mean(1) <= z_near
        else:
            dropped = (zc[tr] <= z_near).any(1)
        u = cam.fx * pc[:, 0] / zc + cam.cx
        w = cam.fy * pc[:, 1] / zc + cam.cy
        if mutant == "swap_xy":
            u, w = w, u
        j, i = np.divmod(np.arange(P), cam.width)
        half = 0.0 if mutant == "centre" else 0.5
        px, py = (i + half)[:, None], (j + half)[:, None]
        U, V, Z = u[tr], w[tr], zc[tr]                                             # [F, 3]
        A = (U[:, 1] - U[:, 0]) * (V[:, 2] - V[:, 0]) - (V[:, 1] - V[:, 0]) * (U[:, 2] - U[:, 0])
        b = []
        for k in range(3):
            k1, k2 = (k + 1) % 3, (k + 2) % 3
            b.append(((U[None, :, k1] - px) * (V[None, :, k2] - py) - (V[None, :, k1] - py) * (U[None, :, k2] - px)) / A[None])
        ok = np.isfinite(A) & (A != 0) & ~dropped
        if mutant == "cull_pos":
            ok &= A < 0
        if mutant == "cull_neg":
            ok &= A > 0
        cover = ok[None] & (b[0] >= 0) & (b[1] >= 0) & (b[2] >= 0)
        if mutant == "affine":
            z = b[0] * Z[None, :, 0] + b[1] * Z[None, :, 1] + b[2] * Z[None, :, 2]
        else:
            z = 1.0 / ((b[0] / Z[None, :, 0] + b[1] / Z[None, :, 1]) + b[2] / Z[None, :, 2])
        z = np.where(cover, z, np.inf)
        if key32 or mutant == "tie_larger":
            ids = np.arange(len(tr), dtype=np.uint64)
            if mutant == "tie_larger":
                ids = ids[::-1].copy()                                             # the larger id makes the smaller word
            word = (z.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[None]
            word = np.where(cover, word, np.uint64(2 ** 64 - 1))
            best = word.min(1) if len(tr) else np.full(P, 2 ** 64 - 1, np.uint64)
            face = np.where(best == np.uint64(2 ** 64 - 1), -1, (best & np.uint64(0xffffffff)).astype(np.int64))
            if mutant == "tie_larger":
                face = np.where(face >= 0, len(tr) - 1 - face, -1)
            depth = np.where(face >= 0, (best >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.inf))
        else:
            face = np.where(cover.any(1), np.argmin(z, 1), -1) if len(tr) else np.full(P, -1)
            depth = z.min(1, initial=np.inf).astype(np.float32)
    return face.astype(np.int64), depth.astype(np.float32), int(dropped.sum())


def agrees(ref, face, depth):
    try:
        rr.check_against(ref, face, depth)
        return True
    except AssertionError:
        return False


def scene(name):
    def build():
        v, t = rr.lumpy_sphere()
        cam = rr.inside_cam() if name == "inside" else rr.generic_cam()
        if name == "twins":
            t = np.concatenate([t, t[::-1]], 0)                                    # every face twice: ids f and 575 - f
        if name == "straddle":
            # one big face in front of view 0 with a vertex behind the camera: its centroid is in front
            m = cam.poses[0].astype(np.float64)
            at = lambda x, y, z: m[:, 3] + m[:, 0] * x + m[:, 1] * y + m[:, 2] * z
            v = np.concatenate([v, np.stack([at(-0.5, -0.4, 1.0), at(0.6, -0.3, 1.2), at(0.0, 0.5, -0.5)])], 0)
            t = np.concatenate([t, [[len(v) - 3, len(v) - 2, len(v) - 1]]], 0)
        return v, t, cam, rr.cast(v, t, cam, Z_NEAR)
    return memo(name, build)


def test_the_two_restatements_agree_and_the_ambiguity_cap_holds():
    for name in ("outside", "inside"):
        v, t, cam, refs = scene(name)
        assert len(t) == 288
        covered = amb = 0
        for view, ref in enumerate(refs):
            face, depth, dropped = project_view(v, t, cam, view, Z_NEAR)
            share, worst = rr.check_against(ref, face, depth, (name, view))
            assert dropped == ref["n_dropped"] and (dropped == 0) == (name == "outside") and share <= CAP
            covered += int((ref["face"] >= 0).sum())
            amb += int(ref["ambiguous"].sum())
            # the hit point lies on the pixel's ray at parameter t, and projects back to the pixel's centre
            hit = ref["hit"][ref["face"] >= 0]
            pc = hit @ w2c_of(cam, view)[:, :3].T + w2c_of(cam, view)[:, 3]
            j, i = np.divmod(np.flatnonzero(ref["face"] >= 0), cam.width)
            assert np.abs(cam.fx * pc[:, 0] / pc[:, 2] + cam.cx - (i + 0.5)).max() < 1e-9
            assert np.abs(pc[:, 2] - ref["t"][ref["face"] >= 0]).max() < 1e-12
        print(f"{name}: {covered} covered pixels of {3 * cam.width * cam.height}, {amb} ambiguous")
        assert covered > 1000


def test_the_binary32_word_decides_ties_for_the_smaller_id():
    v, t, cam, refs = scene("twins")
    for view, ref in enumerate(refs):
        face, depth, _ = project_view(v, t, cam, view, Z_NEAR, key32=True)
        rr.check_against(ref, face, depth, ("twins", view))
        hit = face >= 0
        assert hit.sum() > 300 and ref["ambiguous"][hit].all()                   # twins are within the key's resolution
        assert (face[hit] < 288).all()                                             # ... and the word picks the smaller id
        assert np.array_equal(ref["face"][hit], face[hit])                         # as the ray cast's own tie rule does
    # without twins the word picks what the float64 depth picks, on every unambiguous pixel
    v, t, cam, refs = scene("outside")
    for view, ref in enumerate(refs):
        face, depth, _ = project_view(v, t, cam, view, Z_NEAR, key32=True)
        rr.check_against(ref, face, depth)


@pytest.mark.parametrize("mutant,names", [("centre", ("outside",)), ("affine", ("inside",)), ("cull_pos", ("outside", "inside")),
                                          ("cull_neg", ("outside", "inside")), ("swap_xy", ("outside",)),
                                          ("centroid_drop", ("straddle",)), ("tie_larger", ("twins",))])
def test_mutants_of_the_definition_are_rejected(mutant, names):
    rejected = False
    for name in names:
        v, t, cam, refs = scene(name)
        for view, ref in enumerate(refs):
            face, depth, dropped = project_view(v, t, cam, view, Z_NEAR, mutant)
            ok = agrees(ref, face, depth) and dropped == ref["n_dropped"]
            if mutant == "tie_larger" and ok:                                      # (a tie is ambiguous: the exact rule)
                ok = np.array_equal(face[face >= 0], ref["face"][face >= 0])
            rejected |= not ok
    assert rejected, mutant
    for name in names:                                                             # the definition itself passes there
        v, t, cam, refs = scene(name)
        for view, ref in enumerate(refs):
            face, depth, dropped = project_view(v, t, cam, view, Z_NEAR)
            rr.check_against(ref, face, depth, (name, view))
            assert dropped == ref["n_dropped"]
    if mutant == "centroid_drop":
        assert scene("straddle")[3][0]["n_dropped"] == 1


def test_source_masks_restatement_and_the_occlusion_mutant():
    v, t, cam, refs = scene("outside")
    face = np.stack([r["face"] for r in refs]).reshape(3, cam.height, cam.width)
    rng = np.random.default_rng(5)
    fs = rng.integers(-1, 6, len(t)).astype(np.int32)
    groups = [[4, 0], [2], []]
    masks, pixels = rr.source_masks(face, fs, 6, groups)
    assert masks.shape == (3, 3, cam.height, cam.width) and pixels.shape == (3, 6)
    for vw in range(3):
        for p in range(face[vw].size):
            f = face[vw].flat[p]
            s = fs[f] if f >= 0 else -1
            want = [float(s in g) for g in groups]
            assert [masks[vw, c].flat[p] for c in range(3)] == want
        for s in range(6):
            assert pixels[vw, s] == int(((face[vw] >= 0) & (fs[np.clip(face[vw], 0, None)] == s)).sum())
    assert masks[:, 2].sum() == 0 and masks.sum(1).max() == 1
    # a mask that ignores occlusion (any face along the ray, not the one in front) marks the far side of the sphere too
    back = np.zeros(len(t), np.int32) - 1
    zc = rr.camera_depth(cam, 0, v[t].mean(1))
    back[zc > np.median(zc)] = 0                                                   # a source on the far half only
    m_front, _ = rr.source_masks(face[:1], back, 1, [[0]])
    o, d = rr.pixel_rays(cam, 0)
    a = v[t[:, 0]]
    with np.errstate(all="ignore"):
        tt, b0, b1, b2 = rr._intersect(o, d, a, v[t[:, 1]] - a, v[t[:, 2]] - a)
    any_hit = ((tt > 0) & (b0 >= 0) & (b1 >= 0) & (b2 >= 0) & (back[None] == 0)).any(1)
    assert any_hit.sum() > 100 + m_front.sum()


def test_header_declares_the_raster_entry_points_and_ctypes_agrees():
    from esr_nerf_amd import _lib, raster, relight
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    # the names only: tests/test_host.py checks every entry's restype and argument types against the header text
    for name in ENTRIES:
        assert name in _lib.EXPORTS and _lib.SIGNATURES[name][0] is ctypes.c_int, name
    assert int(re.search(r"#define ESR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == _lib.lib().esr_abi_version()
    assert int(re.search(r"#define ESR_RELIGHT_MAX_COND (\d+)", header).group(1)) == relight.MAX_CONDITIONS
    assert raster.BIG_PX >= 1 and raster.Z_NEAR > 0


def test_entry_points_check_their_arguments_before_any_launch():
    """Every code here is returned by the host-side checks: no pointer is read and nothing is launched"""
    from esr_nerf_amd import _lib
    L = _lib.lib()
    null, p, odd = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    cam = _lib.EsrCamera(50.0, 50.0, 18.5, 14.5, 37, 29, 3)

    def faces(cam=cam, w2c=p, v0=0, v1=3, verts=p, nv=5, tris=p, nf=4, z_near=1e-6, big=64, zbuf=p, drop=p, queue=p, cap=12,
              count=p):
        return L.esr_raster_faces(ctypes.byref(cam) if cam else null, w2c, v0, v1, verts, nv, tris, nf, z_near, big, zbuf, drop,
                                  queue, cap, count, null)

    for kw in (dict(cam=None), dict(v0=-1), dict(v0=2, v1=1), dict(v1=4), dict(nv=-1), dict(nf=-1), dict(z_near=0.0),
               dict(z_near=-1.0), dict(z_near=float("nan")), dict(z_near=float("inf")), dict(big=-1), dict(cap=-1), dict(w2c=null),
               dict(zbuf=null), dict(drop=null), dict(verts=null), dict(tris=null), dict(queue=null), dict(count=null),
               dict(zbuf=odd), dict(w2c=odd), dict(verts=odd), dict(tris=odd), dict(queue=odd), dict(count=odd), dict(nv=0),
               dict(cam=_lib.EsrCamera(50.0, 50.0, 1.0, 1.0, 0, 29, 3)), dict(cam=_lib.EsrCamera(0.0, 50.0, 1.0, 1.0, 37, 29, 3)),
               dict(cam=_lib.EsrCamera(50.0, 50.0, 1.0, 1.0, 1 << 12, 1 << 12, 1 << 7))):
        assert faces(**kw) == -1, kw
    for kw in (dict(cap=11), dict(nf=1 << 31, cap=1 << 40), dict(nv=1 << 31)):
        assert faces(**kw) == -2, kw
    assert faces(v0=2, v1=2, w2c=null, zbuf=null, drop=null) == 0                  # an empty range touches nothing
    for args, code in (((p, -1, p, p, null), -1), ((null, 5, p, p, null), -1), ((p, 5, null, p, null), -1), ((p, 5, p, null, null), -1),
                       ((odd, 5, p, p, null), -1), ((p, 1 << 31, p, p, null), -2), ((null, 0, null, null, null), 0)):
        assert L.esr_raster_resolve(*args) == code, args

    def masks(face=p, nv=2, npx=100, fs=p, nf=7, cond=p, S=3, nc=2, out=p, pix=p):
        return L.esr_source_masks(face, nv, npx, fs, nf, cond, S, nc, out, pix, null)

    for kw in (dict(nv=-1), dict(npx=-1), dict(nf=-1), dict(S=-1), dict(nc=-1), dict(face=null), dict(fs=null), dict(cond=null),
               dict(out=null), dict(pix=null), dict(pix=odd), dict(face=ctypes.c_void_p(0x1002))):
        assert masks(**kw) == -1, kw
    for kw in (dict(nc=17), dict(nv=1 << 16, npx=1 << 16), dict(nf=1 << 31)):
        assert masks(**kw) == -2, kw
    assert masks(nv=0, face=null, out=null, pix=null) == 0


class _Report:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def _blender_cams(width=8, height=6, n=3, seed=0):
    from esr_nerf_amd.camera import Cameras
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, 4, 4))
    M[:, 3] = [0, 0, 0, 1]
    return Cameras.from_blender(M, 0.7, width, height), M


def test_edit_view_data_refusals_and_the_pose_round_trip():
    from esr_nerf_amd import raster
    from esr_nerf_amd.camera import Cameras
    cams, M = _blender_cams()
    for v in range(3):                                                             # float32(matrix), bit for bit
        assert np.array_equal(raster.blender_pose(cams, v).numpy(), M[v].astype(np.float32))
    with pytest.raises(ValueError):
        raster.blender_pose(cams, 3)
    # what label_edit_rays inverts is the pose whose float64 inverse the rasteriser uses, up to the sign flip
    w = raster.world_to_camera(cams)
    assert w.shape == (3, 12) and w.dtype == np.float64
    m4 = np.eye(4)
    m4[:3] = cams.poses[1].numpy().astype(np.float64)
    assert np.abs(w[1].reshape(3, 4) @ m4 - np.eye(4)[:3]).max() < 1e-12
    off = dict(sources=[0], mode="off")
    poses = cams.poses
    for bad, word in ((Cameras(poses, 50.0, 51.0, 4.0, 3.0, 8, 6), "focal"), (Cameras(poses, 50.0, 50.0, 4.5, 3.0, 8, 6), "centre"),
                      (Cameras(poses, 50.0, 50.0, 4.0, 2.5, 8, 6), "centre")):
        with pytest.raises(ValueError, match=word):
            raster.edit_view_data(None, _Report(2), bad, 0, [off])
    rep = _Report(3)
    for edits in ([], [dict(sources=[0], mode="on")], [dict(sources=[0], mode="dim")], [dict(sources=[3], mode="off")],
                  [dict(sources=[-1], mode="off")], [dict(sources=[1], mode="off"), dict(sources=[0, 1], mode="i_change")],
                  [dict(sources=[0], mode="c_change", color=(1, 2, 3, 4))], [dict(sources=[], mode="off")] * 17):
        with pytest.raises(ValueError):
            raster.edit_view_data(None, rep, cams, 0, edits)
    with pytest.raises(ValueError):
        raster.edit_view_data(None, rep, cams, 3, [off])
    with pytest.raises(ValueError, match="twice"):
        raster.source_masks(torch.zeros(1, 2, 2, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), 3, [[1], [1]])
    with pytest.raises(ValueError):
        raster.source_masks(torch.zeros(1, 2, 2, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), 3, [[3]])
    # CPU tensors raise: there is no CPU kernel
    with pytest.raises(RuntimeError, match="no CPU kernel"):
        raster.rasterize(torch.zeros(3, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.int64), cams)
    with pytest.raises(RuntimeError, match="no CPU kernel"):
        raster.source_masks(torch.zeros(1, 2, 2, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), 3, [[1]])
