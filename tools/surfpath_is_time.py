"""Times and errors of the importance-sampled path tracer (esr_nerf_amd/sources.py: path_light(sampling="brdf"),
csrc/surfpath_is.hip) beside the uniform one (csrc/surfpath.hip) on the surface and the two views of tools/surfpath_time.py -- the
marching-cubes mesh of a ``--lattice``^3 analytic field with two sources, "outside" (view 0 of the ring: most paths are one
segment long) and "inside" (a camera within the inner shell: a closed cavity, every path runs until something ends it; no sky
and none of the outer shell's sources reach it, so here two caps of the inner shell are the sources) -- under a seeded 48-lobe
environment, for the surface's own material ("varied": roughness 0.2 .. 0.9) and, in the cavity, for two uniform
ones: "diffuse" (roughness 1, metallic 0) and "glossy" (roughness 0.1, metallic 1).

    python tools/surfpath_is_time.py [--size 800] [--lattice 512] [--paths 16 64] [--depths 1 2 4] [--repeats 3] [--out profiles/surfpath_is_time.json]

Per (view, material, N, D), in the same run on the same inputs and in turn (device events after a warm-up; median and minimum):
``esr_surface_path`` (uniform), ``esr_surface_path_is`` without roulette, and with ``rr_start = 2``.  For each the milliseconds, the
segments a path casts on average and the segments per second (from ``trace`` on every ``--stat-stride``-th hit pixel), the share
of paths by their end code, and on every ``--ref-stride``-th hit pixel the RMSE of the sum of the three components against a
``--ref-paths``-path image of the new entry at the same depth without roulette (another seed); the equal-error ratio
(RMSE_u / RMSE_b)^2 (t_u / t_b) says how much longer the uniform sampler takes to reach the new entry's error.  Also the peak
device memory, and the registers and waves per SIMD of the four kernels from the device assembly.  One JSON object, printed and
written to ``--out``.  No number here is a pass condition.
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

from raster_time import HBM_TBS, clock_state, ring_cameras, surface  # noqa: E402
from surflight_time import Report, alternate, attributes, peak_mb  # noqa: E402
from surfpath_time import centre_camera  # noqa: E402


class CavityReport:
    """two sources on the INNER shell, the caps z > 0.3 and x > 0.3: the lamps of the closed cavity, which neither the sky nor
    the outer shell's sources of surflight_time.Report reach"""

    def __init__(self, verts, tris):
        c = verts[tris].mean(1)
        inner = c.norm(dim=1) <= 0.7
        fs = torch.full((tris.shape[0],), -1, dtype=torch.int32, device=verts.device)
        fs[inner & (c[:, 2] > 0.3)] = 0
        fs[inner & (c[:, 0] > 0.3) & (c[:, 2] <= 0.3)] = 1
        self.face_source = fs
        a, b, cc = (verts[tris[:, k]] for k in range(3))
        area = torch.linalg.cross(b - a, cc - a).norm(dim=1) * 0.5
        self.area = torch.stack([area[fs == s].sum() for s in range(2)])

    def __len__(self):
        return 2


VARIANTS = {"uniform": dict(), "brdf": dict(sampling="brdf"), "brdf_rr2": dict(sampling="brdf", roulette=2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--lattice", type=int, default=512)
    ap.add_argument("--paths", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--depths", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--stat-stride", type=int, default=64)
    ap.add_argument("--ref-stride", type=int, default=256)
    ap.add_argument("--ref-paths", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surfpath_is_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("surfpath_is_time.py measures on the GPU; none is visible")
    import kernel_meta as km
    from esr_nerf_amd import raycast, sources
    from esr_nerf_amd.esrnerf import SphericalGaussian
    dev = torch.device("cuda:0")
    res = dict(size=args.size, lattice=args.lattice, repeats=args.repeats, ref_paths=args.ref_paths, ref_stride=args.ref_stride,
               device=torch.cuda.get_device_name(0), hbm_copy_rate_tbs=HBM_TBS, clock_state_before=clock_state())
    verts, tris = surface(args.lattice, dev)
    V = verts.shape[0]
    res.update(vertices=int(V), faces=int(tris.shape[0]), sources=2)
    torch.manual_seed(0)
    sg = SphericalGaussian(48).to(dev)
    env = tuple(p.detach().float().reshape(48, -1).squeeze(-1).contiguous() for p in (sg.mus, sg.lambdas, sg.lobes))
    bvh = raycast.build(verts, tris)
    seed = 20261021
    for view, cams, rep, mats in (("outside", ring_cameras(100, args.size, dev), Report(verts, tris), ("varied",)),
                                  ("inside", centre_camera(args.size, dev), CavityReport(verts, tris), ("varied", "diffuse", "glossy"))):
        varied = attributes(verts, tris, rep.face_source)
        uniform_mat = lambda ro, me: dict(varied, roughness=torch.full((V,), ro, device=dev), metallic=torch.full((V,), me, device=dev))
        materials = {"varied": varied, "diffuse": uniform_mat(1.0, 0.0), "glossy": uniform_mat(0.1, 1.0)}
        o, d, _ = raycast.pixel_rays(cams, 0)
        hit = raycast.cast(bvh, o, d)
        got_px = hit.face >= 0
        hit_ids = torch.nonzero(got_px)[:, 0]
        for mname in mats:
            surf = sources.Surface(verts, tris, materials[mname])
            lights = sources.source_lights(surf, rep, 16)
            x, n, a, wo = sources._hit_points(surf, hit, d)
            pts = (x, n, hit.face, a["basecolor"].contiguous(), a["roughness"][:, 0].contiguous(), a["metallic"][:, 0].contiguous(), wo)
            sub = lambda stride: [t[hit_ids[::stride]].contiguous() for t in pts]
            stat, ref_pts = sub(args.stat_stride), sub(args.ref_stride)
            total = lambda r: r["env_dir"].double() + r["env_indir"].double() + r["src_indir"].double()
            out = res[f"{view}_{mname}"] = dict(pixels=int(x.shape[0]), pixels_hit=int(got_px.sum()), ref_pixels=int(ref_pts[0].shape[0]))
            for D in args.depths:
                common = dict(env=env, depth=D, bvh=bvh, lights=lights)
                ref = total(sources.path_light(surf, rep, *ref_pts, paths=args.ref_paths, seed=seed + 1, sampling="brdf", **common))
                scale = float(ref.abs().mean())
                for N in args.paths:
                    calls = {k: (lambda kw=kw: sources.path_light(surf, rep, *pts, paths=N, seed=seed, **common, **kw)) for k, kw in VARIANTS.items()}
                    ms = alternate(calls, args.repeats, warmup=1)
                    row = {}
                    for k, kw in VARIANTS.items():
                        _, mb = peak_mb(calls[k])
                        part = sources.path_light(surf, rep, *stat, paths=N, seed=seed, return_trace=True, **common, **kw)
                        cast = float((part["trace"] > -2).sum())
                        per_path = cast / part["end"].numel()
                        est = total(sources.path_light(surf, rep, *ref_pts, paths=N, seed=seed, **common, **kw))
                        rmse = float(torch.sqrt(((est - ref) ** 2).mean()))
                        sec = ms[k][0] * 1e-3
                        row[k] = dict(ms_median_min=ms[k], peak_mb=mb, segments_per_path=round(per_path, 3),
                                      msegments_per_s=round(per_path * N * float(got_px.sum()) / sec / 1e6, 1),
                                      ends_share=[round(float((part["end"] == c).float().mean()), 4) for c in range(5)],
                                      rmse=rmse, rmse_over_mean=round(rmse / scale, 4) if scale > 0 else None)
                    for k in ("brdf", "brdf_rr2"):
                        u, b = row["uniform"], row[k]
                        row[k]["equal_error_ratio"] = round((u["rmse"] / b["rmse"]) ** 2 * (u["ms_median_min"][0] / b["ms_median_min"][0]), 3) \
                            if b["rmse"] > 0 else None
                    out[f"paths_{N}_depth_{D}"] = row
                    print(f"{view}_{mname}", f"paths_{N}_depth_{D}", json.dumps(row), flush=True)
    res["kernels"] = {}
    for f in ("surfpath.hip", "surfpath_is.hip"):
        meta = km.kernel_meta(km.asm_of(os.path.join(ROOT, "esr_nerf_amd", "csrc", f)))
        res["kernels"].update({re.search(r"(\w+_kernel)", km.demangle(k)).group(1): dict(
            vgpr=m.get("vgpr"), scratch=m.get("scratch", 0), lds=m.get("lds", 0), sgpr_spills=m.get("spill_s", 0), waves_per_simd=m.get("occupancy"))
            for k, m in meta.items()})
    res["clock_state_after"] = clock_state()
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
