"""Times of the environment light on the surface (esr_nerf_amd/sources.py: environment_light / vertex_env_radiance,
csrc/surfenv.hip) on the surface tools/raster_time.py builds -- the marching-cubes mesh of a ``--lattice``^3 analytic field,
2.5 M faces at 512 -- for the size^2 pixels of view 0 of raster_time's ring, under a seeded 48-lobe environment.

    python tools/surfenv_time.py [--size 800] [--lattice 512] [--dirs 16 128 256] [--repeats 5] [--out profiles/surfenv_time.json]

By device events after a warm-up (median and minimum), the fused call and the baseline ALTERNATING in one process, per table
size R:
  fused            ``environment_light`` (mode 0) at the view's hit points, without a vertex radiance (the any-hit walk) and
                   with one (the nearest-hit walk)
  composed         the same [P, 3] from the parent's public calls: the flip in torch, ``raycast.occluded`` / ``raycast.cast``
                   over all P R rays in pieces of ``CHUNK`` rays, the environment and the BRDF in float32 torch, the mean in
                   float64; its peak device memory beside the fused call's
and what the kernel asks of the machine: the share of rays that leave the mesh, the boxes and triangles tested per ray (an
``esr_bvh_cast`` pass with ``stats`` over the rays of every ``--stat-stride``-th hit pixel, not the product kernel), the node
bytes that implies against the measured HBM copy rate -- the roof is the chain of dependent node loads, as DESIGN section 4
found for the walk -- and the registers and waves per SIMD of the four kernels from the device assembly.  Then
``vertex_env_radiance`` on the surface simplified to ``--small`` faces.  One JSON object, printed and written to ``--out``.
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
from surflight_time import alternate, attributes, disney32, peak_mb  # noqa: E402

CHUNK = 1 << 22                                       # most rays of one launch of the composed path


def environment32(env, w):
    """the environment along w [..., 3] in float32 torch operations"""
    mus, lam, lobes = env
    unit = lobes / lobes.norm(dim=1, keepdim=True).clamp(min=1e-12)
    e = torch.exp(lam.abs()[None] * (w.reshape(-1, 3) @ unit.T - 1.0))
    return torch.nn.functional.softplus(e @ mus).reshape(*w.shape[:-1], 3)


def composed(bvh, env, table, x, n, face, base, rough, metal, wo, vrad=None, t_min=1e-6):
    """float32 [P, 3] as ``environment_light`` gives it, from the parent's public calls"""
    from esr_nerf_amd import raycast
    P, R = int(x.shape[0]), int(table.shape[0])
    out = torch.empty(P, 3, dtype=torch.float32, device=x.device)
    step = max(1, CHUNK // R)
    tris = bvh.triangles.reshape(-1, 3)
    for p0 in range(0, P, step):
        sl = slice(p0, p0 + step)
        nn = n[sl]
        m = int(nn.shape[0])
        w = table[None].expand(m, R, 3)
        s = (w[..., 0] * nn[:, None, 0] + w[..., 1] * nn[:, None, 1]) + w[..., 2] * nn[:, None, 2]
        w = torch.where((s < 0)[..., None], -w, w)
        o = x[sl][:, None, :].expand(m, R, 3).reshape(-1, 3)
        d = w.reshape(-1, 3).double()
        skip = face[sl][:, None].expand(m, R).reshape(-1).contiguous()
        if vrad is None:
            miss = raycast.occluded(bvh, o, d, t_min, float("inf"), skip_face=skip).reshape(m, R) == 0
            L = environment32(env, w) * miss[..., None]
        else:
            h = raycast.cast(bvh, o, d, t_min, float("inf"), skip_face=skip)
            miss = (h.face < 0).reshape(m, R)
            tri = tris[h.face.clamp(min=0).long()]
            u, v = h.bary[:, 0:1], h.bary[:, 1:2]
            Lh = (((1.0 - u) - v) * vrad[tri[:, 0]].double() + u * vrad[tri[:, 1]].double()) + v * vrad[tri[:, 2]].double()
            L = torch.where(miss[..., None], environment32(env, w).double(), Lh.reshape(m, R, 3))
        Rf = disney32(base[sl][:, None], rough[sl][:, None], metal[sl][:, None], nn[:, None], w, wo[sl][:, None])
        out[sl] = ((L.double() * Rf.double()).sum(1) / R).float()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--lattice", type=int, default=512)
    ap.add_argument("--dirs", type=int, nargs="+", default=[16, 128, 256])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--small", type=int, default=100000)
    ap.add_argument("--stat-stride", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surfenv_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("surfenv_time.py measures on the GPU; none is visible")
    import kernel_meta as km
    from esr_nerf_amd import raycast, sources
    from esr_nerf_amd.esrnerf import SphericalGaussian
    dev = torch.device("cuda:0")
    res = dict(size=args.size, lattice=args.lattice, repeats=args.repeats, device=torch.cuda.get_device_name(0),
               hbm_copy_rate_tbs=HBM_TBS, clock_state_before=clock_state())
    verts, tris = surface(args.lattice, dev)
    surf = sources.Surface(verts, tris, attributes(verts, tris, torch.full((tris.shape[0],), -1, dtype=torch.int32, device=dev)))
    res.update(vertices=int(verts.shape[0]), faces=int(tris.shape[0]))
    torch.manual_seed(0)
    sg = SphericalGaussian(48).to(dev)
    env = tuple(p.detach().float().reshape(48, -1).squeeze(-1).contiguous() for p in (sg.mus, sg.lambdas, sg.lobes))
    bvh = raycast.build(verts, tris)
    cams = ring_cameras(100, args.size, dev)
    o, d, _ = raycast.pixel_rays(cams, 0)
    hit = raycast.cast(bvh, o, d)
    x, n, a, wo = sources._hit_points(surf, hit, d)
    base, rough, metal = a["basecolor"].contiguous(), a["roughness"][:, 0].contiguous(), a["metallic"][:, 0].contiguous()
    got_px = hit.face >= 0
    P = int(x.shape[0])
    res.update(pixels=P, pixels_hit=int(got_px.sum()))
    vrad = sources.vertex_env_radiance(surf, env, 16, bvh=bvh)
    for R in args.dirs:
        table = sources.hemisphere_directions(R, dev)
        kw = dict(dirs=table, faces=hit.face, bvh=bvh)
        mat = (base, rough, metal, wo)
        fused = lambda: sources.environment_light(surf, env, x, n, *mat, **kw)
        fused_rad = lambda: sources.environment_light(surf, env, x, n, *mat, vertex_radiance=vrad, **kw)
        comp = lambda: composed(bvh, env, table, x, n, hit.face, *mat)
        comp_rad = lambda: composed(bvh, env, table, x, n, hit.face, *mat, vrad=vrad)
        reps = max(2, args.repeats * 16 // max(R, 16)) if R > 16 else args.repeats
        ms = alternate(dict(fused=fused, fused_radiance=fused_rad, composed=comp, composed_radiance=comp_rad), reps, warmup=1)
        got, fused_mb = peak_mb(fused)
        got_rad, fused_rad_mb = peak_mb(fused_rad)
        want, comp_mb = peak_mb(comp)
        want_rad, comp_rad_mb = peak_mb(comp_rad)
        _, share = sources.environment_light(surf, env, x, n, *mat, return_open=True, **kw)
        # the walk's work on a sample of the hit pixels: the flipped rays through esr_bvh_cast with stats
        ids = torch.nonzero(got_px)[:: args.stat_stride, 0]
        w = table[None].expand(len(ids), R, 3)
        s = (w[..., 0] * n[ids][:, None, 0] + w[..., 1] * n[ids][:, None, 1]) + w[..., 2] * n[ids][:, None, 2]
        w = torch.where((s < 0)[..., None], -w, w).reshape(-1, 3).double()
        so = x[ids][:, None, :].expand(len(ids), R, 3).reshape(-1, 3)
        sk = hit.face[ids][:, None].expand(len(ids), R).reshape(-1).contiguous()
        stats = {}
        for name, any_hit in (("any_hit", True), ("nearest_hit", False)):
            r = raycast._cast("surfenv_time", bvh, so, w, 1e-6, float("inf"), sk, any_hit, stats=True)
            st = r[1] if any_hit else r.stats
            stats[name] = [round(float(v), 2) for v in st.double().mean(0)]
        rays = int(got_px.sum()) * R
        sec, sec_rad = ms["fused"][0] * 1e-3, ms["fused_radiance"][0] * 1e-3
        node_bytes = rays * 64 * stats["any_hit"][0] / 2
        scale, scale_rad = float(want[got_px].abs().max()), float(want_rad[got_px].abs().max())
        res[f"dirs_{R}"] = dict(
            rays=rays, repeats=reps, open_share_of_hit_pixels=round(float(share[got_px].mean()), 4),
            fused_ms_median_min=ms["fused"], fused_radiance_ms_median_min=ms["fused_radiance"],
            composed_ms_median_min=ms["composed"], composed_radiance_ms_median_min=ms["composed_radiance"],
            speedup=round(ms["composed"][0] / ms["fused"][0], 2), speedup_radiance=round(ms["composed_radiance"][0] / ms["fused_radiance"][0], 2),
            fused_peak_mb=fused_mb, fused_radiance_peak_mb=fused_rad_mb, composed_peak_mb=comp_mb, composed_radiance_peak_mb=comp_rad_mb,
            composed_chunk_rays=CHUNK, unchunked_ray_arrays_gb=round(P * R * 48 / 2 ** 30, 1),
            max_abs_difference_over_max=round(float((got - want)[got_px].abs().max()) / max(scale, 1e-30), 9),
            max_abs_difference_over_max_radiance=round(float((got_rad - want_rad)[got_px].abs().max()) / max(scale_rad, 1e-30), 9),
            mrays_per_s=round(rays / sec / 1e6, 1), mrays_per_s_radiance=round(rays / sec_rad / 1e6, 1),
            boxes_triangles_per_ray=stats, node_bytes_any_hit=int(node_bytes),
            share_of_hbm_copy_rate=round(node_bytes / sec / (HBM_TBS * 1e12), 4))
        print(f"dirs_{R}", json.dumps(res[f"dirs_{R}"]), flush=True)
    small, _ = sources.simplify_surface(surf, target_faces=args.small)
    small_bvh = raycast.build(small.vertices, small.triangles)
    res["vertex_env_radiance"] = dict(faces=int(small.triangles.shape[0]), vertices=int(small.vertices.shape[0]), dirs=128,
                                      ms_median_min=timed(lambda: sources.vertex_env_radiance(small, env, 128, bvh=small_bvh),
                                                          args.repeats, warmup=1))
    meta = km.kernel_meta(km.asm_of(os.path.join(ROOT, "esr_nerf_amd", "csrc", "surfenv.hip")))
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
