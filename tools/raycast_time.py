"""Times of the ray caster (esr_nerf_amd/raycast.py, csrc/bvh.hip) on the surface tools/raster_time.py builds: the
marching-cubes mesh of a ``--lattice``^3 analytic field, 2.5 M faces at 512.

    python tools/raycast_time.py [--size 800] [--lattice 512] [--points 100000] [--repeats 10] [--out profiles/raycast_time.json]

By device events after a warm-up (median and minimum of ``--repeats``):
  build          esr_bvh_keys, torch's stable sort, esr_bvh_tree, esr_bvh_fit, and ``raycast.build`` as a whole
  view           the size^2 pixel rays of view 0 of raster_time's ring: nearest hit and any hit, rays per second, the mean
                 boxes and triangles tested per ray (``stats``), beside ``raster.rasterize`` of the same view
  random         as many rays from a sphere around the mesh towards random points of the unit ball: no two neighbouring
                 lanes walk the same nodes
  visibility     ``sources.source_visibility`` of ``--points`` points between the two shells for two sources of the outer
                 shell, 16 samples each
and, for the limit the walk sits under: the bytes a ray's walk asks for (64 per node record -- two boxes are tested per
record on the way down, one on the way back -- and 96 per triangle: three indices and nine coordinates), the rate that
implies against the measured HBM copy rate, and the binary64 operations of the box and triangle tests against the vector
FP64 peak.  One JSON object, printed and written to ``--out``.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from raster_time import HBM_TBS, clock_state, ring_cameras, surface, timed  # noqa: E402

FP64_VECTOR_TFLOPS = 78.6                            # MI355X vector FP64 peak (the published figure, not measured here)
FLOP_PER_BOX, FLOP_PER_TRI = 6 * 2 + 3 * 5 + 12, 3 * 9 + 3 * 6 + 4 * 5 + 3 + 2      # as csrc/bvh.hip writes them (divisions as one)


class TwoSources:
    """two sources on the outer shell: the caps z > 0.6 and x > 0.6"""

    def __init__(self, verts, tris):
        c = verts[tris].mean(1)
        outer = c.norm(dim=1) > 0.7
        fs = torch.full((tris.shape[0],), -1, dtype=torch.int32, device=verts.device)
        fs[outer & (c[:, 2] > 0.6)] = 0
        fs[outer & (c[:, 0] > 0.6) & (c[:, 2] <= 0.6)] = 1
        self.face_source = fs

    def __len__(self):
        return 2


def build_passes(verts, tris, repeats):
    from esr_nerf_amd import _lib, raycast
    L, dev = _lib.lib(), verts.device
    s = _lib.stream_ptr(dev)
    n_v, n_f = int(verts.shape[0]), int(tris.shape[0])
    b = raycast.build(verts, tris)
    keys = torch.empty(n_f, dtype=torch.int64, device=dev)
    boxes = torch.empty(n_f, 6, dtype=torch.float32, device=dev)
    nodes, lp = torch.empty_like(b.nodes), torch.empty_like(b.leaf_parent)
    counters, root = torch.empty(n_f - 1, dtype=torch.int32, device=dev), torch.empty(6, dtype=torch.float32, device=dev)
    out = {
        "keys": timed(lambda: _lib.check(L.esr_bvh_keys(_lib.ptr(verts), n_v, _lib.ptr(tris), n_f, _lib.ptr(b.scene_box),
                                                        _lib.ptr(keys), _lib.ptr(boxes), s), "keys"), repeats),
        "sort": timed(lambda: torch.sort(keys, stable=True), repeats),
        "tree": timed(lambda: _lib.check(L.esr_bvh_tree(_lib.ptr(b.keys), _lib.ptr(b.order), n_f, _lib.ptr(nodes), _lib.ptr(lp), s),
                                         "tree"), repeats),
        "fit": timed(lambda: _lib.check(L.esr_bvh_fit(_lib.ptr(nodes), _lib.ptr(lp), _lib.ptr(b.order), _lib.ptr(boxes), n_f,
                                                      _lib.ptr(counters), _lib.ptr(root), s), "fit"), repeats),
        "raycast.build": timed(lambda: raycast.build(verts, tris), repeats),
    }
    assert torch.equal(nodes, b.nodes)
    return b, dict(ms_median_min=out, node_bytes=int(b.nodes.numel()) * 4)


def cast_rates(bvh, o, d, repeats):
    from esr_nerf_amd import raycast
    n = int(o.shape[0])
    near = timed(lambda: raycast.cast(bvh, o, d), repeats)
    anyh = timed(lambda: raycast.occluded(bvh, o, d, 0.0, math.inf), repeats)
    h = raycast.cast(bvh, o, d, stats=True)
    st = h.stats.double().mean(0)
    boxes, tri = float(st[0]), float(st[1])
    # a record per two boxes on the way down, per one on the way back: between boxes / 2 and boxes records
    need = n * (64 * boxes / 2 + 96 * tri)
    flop = n * (FLOP_PER_BOX * boxes + FLOP_PER_TRI * tri)
    sec = near[0] * 1e-3
    return dict(rays=n, hit_share=round(float((h.face >= 0).double().mean()), 4),
                nearest_ms_median_min=near, any_hit_ms_median_min=anyh,
                nearest_mrays_per_s=round(n / sec / 1e6, 1), any_hit_mrays_per_s=round(n / (anyh[0] * 1e-3) / 1e6, 1),
                boxes_per_ray=round(boxes, 2), triangles_per_ray=round(tri, 2), most_boxes=int(h.stats[:, 0].max()),
                bytes_asked_at_least=int(need), share_of_hbm_copy_rate=round(need / sec / (HBM_TBS * 1e12), 4),
                fp64_flop=int(flop), share_of_vector_fp64_peak=round(flop / sec / (FP64_VECTOR_TFLOPS * 1e12), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--lattice", type=int, default=512)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("raycast_time.py measures on the GPU; none is visible")
    from esr_nerf_amd import raster, raycast, sources
    dev = torch.device("cuda:0")
    res = dict(size=args.size, lattice=args.lattice, repeats=args.repeats, device=torch.cuda.get_device_name(0),
               hbm_copy_rate_tbs=HBM_TBS, fp64_vector_tflops=FP64_VECTOR_TFLOPS, clock_state_before=clock_state())
    verts, tris = surface(args.lattice, dev)
    res.update(vertices=int(verts.shape[0]), faces=int(tris.shape[0]))
    bvh, res["build"] = build_passes(verts, tris, args.repeats)
    cams = ring_cameras(100, args.size, dev)
    o, d, _ = raycast.pixel_rays(cams, 0)
    res["view"] = cast_rates(bvh, o, d, args.repeats)
    res["view"]["rasterize_ms_median_min"] = timed(lambda: raster.rasterize(verts, tris, cams, views=0), args.repeats)
    r = raster.rasterize(verts, tris, cams, views=0)
    f, _ = raycast.cast_cameras(bvh, cams, views=0)
    res["view"]["pixels_where_the_two_faces_differ"] = int((f != r.face).sum())
    g = torch.Generator(device=dev).manual_seed(0)
    n = args.size * args.size
    a = torch.randn(n, 3, dtype=torch.float64, device=dev, generator=g)
    ro = 3.0 * a / a.norm(dim=1, keepdim=True)
    b = torch.randn(n, 3, dtype=torch.float64, device=dev, generator=g)
    target = b / b.norm(dim=1, keepdim=True) * torch.rand(n, 1, dtype=torch.float64, device=dev, generator=g) ** (1 / 3)
    res["random"] = cast_rates(bvh, ro, (target - ro).contiguous(), args.repeats)
    surf, rep = sources.Surface(verts, tris, {}), TwoSources(verts, tris)
    p = torch.randn(args.points, 3, dtype=torch.float64, device=dev, generator=g)
    p = p / p.norm(dim=1, keepdim=True) * (0.6 + 0.2 * torch.rand(args.points, 1, dtype=torch.float64, device=dev, generator=g))
    ms = timed(lambda: sources.source_visibility(surf, rep, p, samples=16, bvh=bvh), max(3, args.repeats // 3), warmup=1)
    vis = sources.source_visibility(surf, rep, p, samples=16, bvh=bvh)
    res["visibility"] = dict(points=args.points, sources=2, samples=16, segments=args.points * 2 * 16, ms_median_min=ms,
                             msegments_per_s=round(args.points * 32 / (ms[0] * 1e-3) / 1e6, 1),
                             mean_share=[round(float(x), 4) for x in vis.mean(0)],
                             source_faces=[int((rep.face_source == s).sum()) for s in range(2)])
    res["clock_state_after"] = clock_state()
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
