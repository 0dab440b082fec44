"""Times of the surface lighting (esr_nerf_amd/sources.py: direct_light / lit_view, csrc/surflight.hip) on the surface
tools/raster_time.py builds -- the marching-cubes mesh of a ``--lattice``^3 analytic field, 2.5 M faces at 512 -- with the two
patches of tools/raycast_time.py marked as sources, for the size^2 pixels of view 0 of raster_time's ring.

    python tools/surflight_time.py [--size 800] [--lattice 512] [--repeats 10] [--out profiles/surflight_time.json]

By device events after a warm-up (median and minimum of ``--repeats``), the fused call and the baseline ALTERNATING in one
process:
  cast_cameras   the nearest hits of the view
  fused          ``direct_light`` (mode 0, per source) at the view's hit points, at 16 and 64 samples per source
  composed       the same [P, S, 3] from the parent's public calls: ``raycast.occluded_segments`` over all P S K segments in
                 pieces of ``sources.VISIBILITY_CHUNK``, the geometric term in torch (float64) and a float32 torch
                 restatement of the BRDF; its peak device memory beside the fused call's
  lit_view       the whole of ``sources.lit_view`` (lights, cast, interpolation, the fused call)
and what the kernel asks of the machine: the segments walked of those offered (``seen``), the boxes and triangles tested per
walked segment (a second any-hit pass with ``stats`` over the walked segments, not the product kernel), the bytes and the
binary64 operations that implies against the measured HBM copy rate and the vector FP64 peak, and the registers and waves
per SIMD of the two kernels from the device assembly.  One JSON object, printed and written to ``--out``.
"""
import argparse
import json
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from raster_time import HBM_TBS, clock_state, ring_cameras, surface, timed  # noqa: E402
from raycast_time import FLOP_PER_BOX, FLOP_PER_TRI, FP64_VECTOR_TFLOPS, TwoSources  # noqa: E402

FLOP_PER_SLOT = 3 + 5 + 1 + 3 + 2 * 5 + 3          # d, r2, sqrt, w, two cosines, G: per offered slot, before the walk
LIGHT_BYTES_PER_SLOT = 24 + 24 + 8 + 12 + 4         # point, normal, weight, radiance, face: from cache after the first wave


class Report(TwoSources):
    """raycast_time's two sources with what source_lights reads of a SourceReport: the areas"""

    def __init__(self, verts, tris):
        super().__init__(verts, tris)
        a, b, c = (verts[tris[:, k]] for k in range(3))
        area = torch.linalg.cross(b - a, c - a).norm(dim=1) * 0.5
        self.area = torch.stack([area[self.face_source == s].sum() for s in range(2)])


def attributes(verts, tris, face_source):
    """per vertex: the normal of the shell (outward on the outer shell, inward on the inner), a material that varies over the
    surface, emission 1 .. 3 at the vertices of source faces"""
    r = verts.norm(dim=1, keepdim=True)
    normal = (verts / r * torch.where(r > 0.7, 1.0, -1.0)).float()
    x, y, z = verts.float().unbind(1)
    em = torch.zeros(verts.shape[0], 3, device=verts.device)
    hot = torch.unique(tris[face_source >= 0])
    em[hot] = torch.stack([2 + torch.sin(5 * x[hot]), 2 + torch.cos(4 * y[hot]), 2 + torch.sin(3 * z[hot])], 1)
    return dict(normal=normal.contiguous(), basecolor=torch.stack([0.5 + 0.4 * torch.sin(3 * x), 0.5 + 0.4 * torch.sin(4 * y),
                                                                   0.5 + 0.4 * torch.sin(5 * z)], 1).contiguous(),
                roughness=(0.55 + 0.35 * torch.sin(6 * x + y)).contiguous(), metallic=(0.5 + 0.5 * torch.sin(2 * z - x)).contiguous(),
                emission=em.contiguous(), sdf=torch.zeros(verts.shape[0], device=verts.device))


def disney32(a, ro, m, n, wi, wo):
    """R [..., 3] of csrc/disney.h in float32 torch operations (forward only)"""
    pi, eps = math.pi, 1e-7
    dot = lambda p, q: (p * q).sum(-1)
    h = wi + wo
    h = h / h.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    noh, ooh = dot(n, h).clamp(min=0), dot(wo, h).clamp(min=0)
    ion, oon = dot(wi, n).clamp(min=0), dot(wo, n).clamp(min=0)
    r2 = (ro * ro).clamp(min=eps)
    D = 1.0 / (r2 * pi) * torch.exp(2.0 / r2 * (noh - 1.0))
    t5 = (1.0 - ooh) ** 5
    k = (1.0 + ro) * (1.0 + ro) / 8.0
    V = (0.5 / (ion * (1.0 - k) + k).clamp(min=eps)) * (0.5 / (oon * (1.0 - k) + k).clamp(min=eps))
    F0 = 0.04 * (1.0 - m[..., None]) + a * m[..., None]
    Fr = F0 + (1.0 - F0) * t5[..., None]
    return ((1.0 - m[..., None]) * a / pi + (D * V)[..., None] * Fr) * (ion * pi * 2.0)[..., None]


def composed(bvh, lights, x, n, base, rough, metal, wo, eps=1e-6):
    """float32 [P, S, 3] as ``direct_light(..., per_source=True)`` gives it, from the parent's public calls"""
    from esr_nerf_amd import raycast, sources
    P, (S, K) = int(x.shape[0]), lights.weight.shape
    y, g, A, E, face = lights.point, lights.normal, lights.weight, lights.radiance, lights.face
    occ = torch.empty(P, S, K, dtype=torch.uint8, device=x.device)
    step = max(1, sources.VISIBILITY_CHUNK // (S * K))
    for p0 in range(0, P, step):
        p = x[p0:p0 + step]
        m = int(p.shape[0])
        occ[p0:p0 + step] = raycast.occluded_segments(bvh, p[:, None, None, :].expand(m, S, K, 3).reshape(-1, 3),
                                                      y[None].expand(m, S, K, 3).reshape(-1, 3),
                                                      skip_face=face[None].expand(m, S, K).reshape(-1), eps=eps).reshape(m, S, K)
    d = y[None] - x[:, None, None, :]
    r2 = (d * d).sum(-1)
    w = d / torch.sqrt(r2)[..., None]
    cos_l = -(g[None] * w).sum(-1)
    cos_x = (n.double()[:, None, None, :] * w).sum(-1)
    live = (A[None] != 0) & (r2 > 0) & (cos_l > 0) & (cos_x > 0) & (occ == 0)
    G = cos_l * A[None] / torch.maximum(r2, A[None].expand_as(r2))
    un = lambda t: t[:, None, None]
    R = disney32(un(base), un(rough), un(metal), un(n), w.float(), un(wo))
    term = R.double() * (1.0 / (2.0 * math.pi)) * G[..., None] * E.double()[None]
    return torch.where(live[..., None], term, torch.zeros_like(term)).sum(2).float()


def alternate(fns, repeats, warmup=2):
    """{name: (median, min) ms}: the calls in turn, `repeats` rounds, by device events"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: (round(sorted(v)[len(v) // 2], 4), round(min(v), 4)) for k, v in ms.items()}


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--lattice", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surflight_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("surflight_time.py measures on the GPU; none is visible")
    import kernel_meta as km
    from esr_nerf_amd import raycast, sources
    dev = torch.device("cuda:0")
    res = dict(size=args.size, lattice=args.lattice, repeats=args.repeats, device=torch.cuda.get_device_name(0),
               hbm_copy_rate_tbs=HBM_TBS, fp64_vector_tflops=FP64_VECTOR_TFLOPS, clock_state_before=clock_state())
    verts, tris = surface(args.lattice, dev)
    rep = Report(verts, tris)
    surf = sources.Surface(verts, tris, attributes(verts, tris, rep.face_source))
    res.update(vertices=int(verts.shape[0]), faces=int(tris.shape[0]),
               source_faces=[int((rep.face_source == s).sum()) for s in range(2)], source_area=[round(float(a), 4) for a in rep.area])
    bvh = raycast.build(verts, tris)
    cams = ring_cameras(100, args.size, dev)
    res["cast_cameras_ms_median_min"] = timed(lambda: raycast.cast_cameras(bvh, cams, 0), args.repeats)
    o, d, _ = raycast.pixel_rays(cams, 0)
    hit = raycast.cast(bvh, o, d)
    x, n, a, wo = sources._hit_points(surf, hit, d)
    base, rough, metal = a["basecolor"].contiguous(), a["roughness"][:, 0].contiguous(), a["metallic"][:, 0].contiguous()
    P = int(x.shape[0])
    res.update(pixels=P, pixels_hit=int((hit.face >= 0).sum()))
    for samples in (16, 64):
        lights = sources.source_lights(surf, rep, samples)
        fused = lambda: sources.direct_light(surf, lights, x, n, base, rough, metal, wo, bvh=bvh, per_source=True)
        base_fn = lambda: composed(bvh, lights, x, n, base, rough, metal, wo)
        ms = alternate(dict(fused=fused, composed=base_fn), args.repeats if samples == 16 else max(3, args.repeats // 3))
        got, fused_mb = peak_mb(fused)
        want, composed_mb = peak_mb(base_fn)
        _, seen = sources.direct_light(surf, lights, x, n, base, rough, metal, wo, bvh=bvh, per_source=True, return_seen=True)
        offered, walked = P * 2 * samples, int((seen > 0).sum())
        ip, is_, ik = torch.nonzero(seen > 0, as_tuple=True)
        po, q = x[ip].contiguous(), lights.point[is_, ik].contiguous()
        _, st = raycast._cast("surflight_time", bvh, po, q - po, 1e-6, 1.0 - 1e-6, lights.face[is_, ik].contiguous(), True, stats=True)
        boxes, tri = (float(v) for v in st.double().mean(0))
        sec = ms["fused"][0] * 1e-3
        need = walked * (64 * boxes / 2 + 96 * tri) + P * (24 + 12 + 12 + 4 + 4 + 12) + P * 2 * 12
        flop = walked * (FLOP_PER_BOX * boxes + FLOP_PER_TRI * tri) + offered * FLOP_PER_SLOT
        scale = float(want.abs().max())
        res[f"samples_{samples}"] = dict(
            segments_offered=offered, segments_walked=walked, walked_share=round(walked / offered, 4),
            unoccluded_share_of_walked=round(float((seen == 1).sum()) / max(walked, 1), 4),
            fused_ms_median_min=ms["fused"], composed_ms_median_min=ms["composed"],
            speedup=round(ms["composed"][0] / ms["fused"][0], 2), fused_peak_mb=fused_mb, composed_peak_mb=composed_mb,
            max_abs_difference_over_max=round(float((got - want).abs().max()) / max(scale, 1e-30), 9),
            msegments_walked_per_s=round(walked / sec / 1e6, 1), boxes_per_walked_segment=round(boxes, 2),
            triangles_per_walked_segment=round(tri, 2), bytes_asked_at_least=int(need),
            light_bytes_from_cache=int(offered * LIGHT_BYTES_PER_SLOT),
            share_of_hbm_copy_rate=round(need / sec / (HBM_TBS * 1e12), 4), fp64_flop=int(flop),
            share_of_vector_fp64_peak=round(flop / sec / (FP64_VECTOR_TFLOPS * 1e12), 4))
    res["lit_view_ms_median_min"] = timed(lambda: sources.lit_view(surf, rep, cams, 0, samples=16, bvh=bvh), max(3, args.repeats // 2), warmup=1)
    meta = km.kernel_meta(km.asm_of(os.path.join(ROOT, "esr_nerf_amd", "csrc", "surflight.hip")))
    res["kernels"] = {re.search(r"(\w+_kernel)", km.demangle(k)).group(1): dict(vgpr=m.get("vgpr"), scratch=m.get("scratch", 0),
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
