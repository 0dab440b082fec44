"""Times of the path-traced light on the surface (esr_nerf_amd/sources.py: path_light, csrc/surfpath.hip) on the surface
tools/raster_time.py builds -- the marching-cubes mesh of a ``--lattice``^3 analytic field, 2.5 M faces at 512, with the two
sources of tools/surflight_time.py -- for the size^2 pixels of two views -- "outside", view 0 of raster_time's ring (93 % of the hemisphere rays leave the mesh, and the shell's radial
shading normals make every second hit a back face: the paths are one segment long), and "inside", a camera at the origin within
the inner shell (a closed cavity: every path runs to its full depth) -- under a seeded 48-lobe environment.

    python tools/surfpath_time.py [--size 800] [--lattice 512] [--paths 16 64] [--depths 1 2 4] [--repeats 3] [--out profiles/surfpath_time.json]

By device events after a warm-up (median and minimum), per (N, D): the milliseconds of ``path_light`` (mode 0, 16 samples per
source), the segments and shadow segments it walked (from ``trace``: a segment that hits and is not a back face gathers one
shadow segment per source whose sample faces the vertex -- an upper bound: the silent slots are counted) and their rate, the share
of paths by the way they end, and the peak device memory.  By depth, on every ``--stat-stride``-th hit pixel: the boxes and
triangles tested per segment, from a replay of the paths through the public calls (the sampler restated in torch,
``esr_bvh_cast`` with ``stats``), which also counts the segments whose face differs from the kernel's ``trace``.  A comparison
point: D = 1 without sources beside ``environment_light`` with a vertex radiance (the nearest-hit walk) at R = N on the same
points.  The registers and waves per SIMD of the two kernels from the device assembly.  One JSON object, printed and written to
``--out``.  No time here is a pass condition.
"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from raster_time import HBM_TBS, clock_state, ring_cameras, surface, timed  # noqa: E402
from surflight_time import Report, alternate, attributes, peak_mb  # noqa: E402

MASK = 0xFFFFFFFF


class NoSource:
    """a report without a source, for the comparison with environment_light"""
    def __init__(self, face_source):
        self.face_source = torch.full_like(face_source, -1)
        self.area = torch.zeros(0, dtype=torch.float64, device=face_source.device)

    def __len__(self):
        return 0


def centre_camera(size, dev):
    """one camera at the origin, inside the inner shell: a closed cavity, every path runs to its full depth"""
    from esr_nerf_amd.camera import Cameras
    pose = torch.tensor([[[0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]]], dtype=torch.float32, device=dev)
    return Cameras(pose, 1.35 * size, 1.35 * size, size / 2, size / 2, size, size)


def philox(c0, c1, c2, c3, key):
    """Philox4x32-10 on int64 tensors holding 32-bit words (a product wraps modulo 2^64: its two words are the right ones)"""
    k0, k1 = key
    for _ in range(10):
        p0, p1 = c0 * 0xD2511F53, c2 * 0xCD9E8D57
        c0, c1, c2, c3 = ((p1 >> 32) & MASK) ^ c1 ^ k0, p1 & MASK, ((p0 >> 32) & MASK) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
    return c0, c1, c2, c3


def sphere(c0, c1, c2, key):
    """float64 [n, 3]: section X's direction of the counters (c0, c1, c2, .)"""
    w = torch.zeros(c0.shape[0], 3, dtype=torch.float64, device=c0.device)
    w[:, 2] = 1.0
    taken = torch.zeros_like(c0, dtype=torch.bool)
    for block in range(8):
        r = philox(c0, c1, c2, torch.full_like(c0, block), key)
        for h in range(2):
            a1, a2 = 2.0 * (r[2 * h].double() * 2.0 ** -32) - 1.0, 2.0 * (r[2 * h + 1].double() * 2.0 ** -32) - 1.0
            s = a1 * a1 + a2 * a2
            ok = ~taken & (s < 1.0)
            q = torch.sqrt((1.0 - s).clamp(min=0.0))
            w = torch.where(ok[:, None], torch.stack([(2.0 * a1) * q, (2.0 * a2) * q, 1.0 - 2.0 * s], 1), w)
            taken |= ok
    return w


def replay(surf, bvh, ids, x, n, face, N, D, seed, trace, t_min=1e-6):
    """boxes and triangles per segment by depth, and the segments whose face differs from the kernel's, for the paths of the
    points `ids`: the segments re-cast through esr_bvh_cast"""
    from esr_nerf_amd import raycast, sources
    dev = x.device
    key = (seed & MASK, seed >> 32)
    m = len(ids)
    pid = ids.repeat_interleave(N)
    sid = torch.arange(N, device=dev).repeat(m)
    px, pn, pf = x[pid].clone(), n[pid].clone(), face[pid].clone()
    alive = torch.ones(m * N, dtype=torch.bool, device=dev)
    out, differ = [], 0
    for b in range(D):
        idx = torch.nonzero(alive)[:, 0]
        if not len(idx):
            break
        w = sphere(pid[idx], sid[idx], torch.full_like(idx, 2 * b), key)
        wi, nn = w.float(), pn[idx]
        s = (wi[:, 0] * nn[:, 0] + wi[:, 1] * nn[:, 1]) + wi[:, 2] * nn[:, 2]
        w = torch.where((s < 0)[:, None], -w, w)
        h = raycast._cast("surfpath_time", bvh, px[idx].contiguous(), w.contiguous(), t_min, float("inf"), pf[idx].contiguous(), False, stats=True)
        differ += int((h.face != trace[pid[idx], sid[idx], b]).sum())
        st = h.stats.double().mean(0)
        got = h.face >= 0
        out.append(dict(depth=b, segments=int(len(idx)), hit_share=round(float(got.float().mean()), 4), boxes=round(float(st[0]), 2),
                        triangles=round(float(st[1]), 2)))
        hx, _, _, _ = sources._hit_points(surf, h, w)
        hwo = -w.float()
        tri = surf.triangles[h.face.clamp(min=0).long()]
        b32 = torch.stack([(1.0 - h.bary[:, 0]) - h.bary[:, 1], h.bary[:, 0], h.bary[:, 1]], 1).float()
        nv = surf.attrs["normal"].float()
        raw = (nv[tri[:, 0]] * b32[:, 0:1] + nv[tri[:, 1]] * b32[:, 1:2]) + nv[tri[:, 2]] * b32[:, 2:3]
        ln = torch.sqrt((raw[:, 0] * raw[:, 0] + raw[:, 1] * raw[:, 1]) + raw[:, 2] * raw[:, 2])
        hn = raw / ln[:, None]
        front = (hn[:, 0] * hwo[:, 0] + hn[:, 1] * hwo[:, 1]) + hn[:, 2] * hwo[:, 2] > 0
        go = got & front & (ln > 0)
        alive[idx[~go]] = False
        keep = idx[go]
        px[keep], pn[keep], pf[keep] = hx[go], hn[go], h.face[go]
    return out, differ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--lattice", type=int, default=512)
    ap.add_argument("--paths", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--depths", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--stat-stride", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surfpath_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("surfpath_time.py measures on the GPU; none is visible")
    import kernel_meta as km
    from esr_nerf_amd import raycast, sources
    from esr_nerf_amd.esrnerf import SphericalGaussian
    dev = torch.device("cuda:0")
    res = dict(size=args.size, lattice=args.lattice, repeats=args.repeats, device=torch.cuda.get_device_name(0),
               hbm_copy_rate_tbs=HBM_TBS, clock_state_before=clock_state())
    verts, tris = surface(args.lattice, dev)
    rep = Report(verts, tris)
    surf = sources.Surface(verts, tris, attributes(verts, tris, rep.face_source))
    res.update(vertices=int(verts.shape[0]), faces=int(tris.shape[0]), sources=len(rep))
    torch.manual_seed(0)
    sg = SphericalGaussian(48).to(dev)
    env = tuple(p.detach().float().reshape(48, -1).squeeze(-1).contiguous() for p in (sg.mus, sg.lambdas, sg.lobes))
    bvh = raycast.build(verts, tris)
    lights = sources.source_lights(surf, rep, 16)
    vrad = sources.vertex_env_radiance(surf, env, 16, bvh=bvh)
    S, seed = len(rep), 20261021
    for view, cams in (("outside", ring_cameras(100, args.size, dev)), ("inside", centre_camera(args.size, dev))):
        o, d, _ = raycast.pixel_rays(cams, 0)
        hit = raycast.cast(bvh, o, d)
        x, n, a, wo = sources._hit_points(surf, hit, d)
        mat = (a["basecolor"].contiguous(), a["roughness"][:, 0].contiguous(), a["metallic"][:, 0].contiguous(), wo)
        got_px = hit.face >= 0
        out = res[view] = dict(pixels=int(x.shape[0]), pixels_hit=int(got_px.sum()))
        ids = torch.nonzero(got_px)[:: args.stat_stride, 0]
        sub = [t[ids].contiguous() for t in (x, n, hit.face) + mat]
        # (the pixels that miss are NaN points: all their paths leave at segment 0 without a walk; only the hit pixels are counted)
        for N in args.paths:
            for D in args.depths:
                kw = dict(env=env, paths=N, depth=D, seed=seed, bvh=bvh, lights=lights)
                call = lambda: sources.path_light(surf, rep, x, n, hit.face, *mat, **kw)
                ms = timed(call, args.repeats, warmup=1)
                _, mb = peak_mb(call)
                # (a sample of the pixels in a call of its own: the counter holds the point's index in ITS call, and the replay follows that call)
                part = sources.path_light(surf, rep, *sub, return_trace=True, **kw)
                tr, end = part["trace"], part["end"]
                cast = tr > -2
                lands = (tr >= 0) & ~((end == 2)[..., None] & (torch.arange(D, device=dev) == cast.sum(-1, keepdim=True) - 1))
                scale = float(got_px.sum()) / len(ids)
                segments, shadows = float(cast.sum()) * scale, float(lands.sum()) * S * scale
                sec = ms[0] * 1e-3
                by_depth, differ = replay(surf, bvh, torch.arange(len(ids), device=dev), sub[0], sub[1], sub[2], N, D, seed, tr)
                out[f"paths_{N}_depth_{D}"] = dict(
                    ms_median_min=ms, peak_mb=mb, segments=int(segments), shadow_segments_at_most=int(shadows),
                    msegments_per_s=round(segments / sec / 1e6, 1), mwalks_per_s_at_most=round((segments + shadows) / sec / 1e6, 1),
                    ends_share=[round(float((end == k).float().mean()), 4) for k in range(3)], boxes_triangles_per_segment_by_depth=by_depth,
                    replayed_segments_with_another_face=differ)
                print(view, f"paths_{N}_depth_{D}", json.dumps(out[f"paths_{N}_depth_{D}"]), flush=True)
            # the comparison point: one segment, no source, beside environment_light's nearest-hit walk at R = N
            bare, table = NoSource(rep.face_source), sources.hemisphere_directions(N, dev)
            cmp_ms = alternate(dict(
                environment_light=lambda: sources.environment_light(surf, env, x, n, *mat, dirs=table, faces=hit.face, vertex_radiance=vrad, bvh=bvh),
                path_light=lambda: sources.path_light(surf, bare, x, n, hit.face, *mat, env=env, paths=N, depth=1, seed=seed, bvh=bvh)), args.repeats, warmup=1)
            out[f"one_segment_{N}"] = dict(rays=int(got_px.sum()) * N, **{k + "_ms_median_min": v for k, v in cmp_ms.items()})
            print(view, f"one_segment_{N}", json.dumps(out[f"one_segment_{N}"]), flush=True)
    meta = km.kernel_meta(km.asm_of(os.path.join(ROOT, "esr_nerf_amd", "csrc", "surfpath.hip")))
    res["kernels"] = {re.search(r"(\w+_kernel)", km.demangle(k)).group(1): dict(vgpr=m.get("vgpr"), scratch=m.get("scratch", 0), lds=m.get("lds", 0),
                                                                              sgpr_spills=m.get("spill_s", 0), waves_per_simd=m.get("occupancy"))
                      for k, m in meta.items()}
    res["clock_state_after"] = clock_state()
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
