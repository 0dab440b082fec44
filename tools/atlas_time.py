"""Times of the texture atlas (esr_nerf_amd/atlas.py, sources.bake_materials; csrc/atlas.hip) on the surface tools/raster_time.py
builds -- the marching-cubes mesh of a ``--lattice``^3 analytic field, 2.5 M faces at 512 -- simplified to ``--faces`` faces.

    python tools/atlas_time.py [--lattice 512] [--faces 100000] [--sizes 2048 4096] [--view 800] [--repeats 9] [--out profiles/atlas_time.json]

By device events after a warm-up (median, minimum and the spread max / min), per atlas size:
  levels          one level pass with its 128-byte read-back (host clock: the read-back is part of it)
  bisect          ``atlas.build`` without the charts and texels: the density search, its level passes counted
  sort            torch's stable sort of the levels
  charts, texels  the two entries through the C ABI on preallocated outputs; the texel pass with and without the 12
                  interpolated channels, as bytes written per second against the float4 copy rate measured in the same run
  bake_model      ``sources.bake_materials`` with the light-transport model of tools/surface_time.py (its grids stand in for a
                  trained model's: the time is that of ``surface_attributes`` at the owned texels plus the scatter)
  sample          ``atlas.sample`` of 11 channels at the nearest hits of an ``--view``^2 camera view
and the peak device memory of ``atlas.build``, the share of texels owned and inside (the fill rate) and the density found.
One JSON object, printed and written to ``--out``.
"""
import argparse
import ctypes
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from raster_time import clock_state, ring_cameras, surface  # noqa: E402
from surflight_time import attributes, peak_mb  # noqa: E402


def timed(fn, repeats, warmup=2):
    """(median, min, max / min) milliseconds of fn() by device events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return [round(ms[len(ms) // 2], 4), round(ms[0], 4), round(ms[-1] / max(ms[0], 1e-9), 2)]


def host_timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return [round(ms[len(ms) // 2], 4), round(ms[0], 4), round(ms[-1] / max(ms[0], 1e-9), 2)]


def copy_rate_tbs(dev, repeats):
    """read + written bytes per second of a 1 GiB device copy"""
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    ms = timed(lambda: dst.copy_(src), repeats)
    return round(2 * src.numel() * 4 / (ms[0] * 1e-3) / 1e12, 3), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=512)
    ap.add_argument("--faces", type=int, default=100000)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--view", type=int, default=800)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--config", default="C4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "atlas_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("atlas_time.py measures on the GPU; none is visible")
    import kernel_meta as km
    from esr_nerf_amd import _lib, atlas, raycast, sources
    from surface_time import build_model
    dev = torch.device("cuda:0")
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    res = dict(lattice=args.lattice, repeats=args.repeats, device=torch.cuda.get_device_name(0), clock_state_before=clock_state())
    res["hbm_copy_rate_tbs"], res["copy_1gib_ms_median_min_spread"] = copy_rate_tbs(dev, args.repeats)
    verts, tris = surface(args.lattice, dev)
    big = sources.Surface(verts, tris, attributes(verts, tris, torch.full((tris.shape[0],), -1, dtype=torch.int32, device=dev)))
    res.update(full_vertices=int(verts.shape[0]), full_faces=int(tris.shape[0]))
    surf, _ = sources.simplify_surface(big, target_faces=args.faces)
    del big, verts, tris
    v, t = surf.vertices, surf.triangles
    F, V = int(t.shape[0]), int(v.shape[0])
    res.update(faces=F, vertices=V)
    model = build_model(args.config, dev)
    bvh = raycast.build(v, t)
    cams = ring_cameras(100, args.view, dev)
    o, d, _ = raycast.pixel_rays(cams, 0)
    hit = raycast.cast(bvh, o, d)
    packed = torch.cat([surf.attrs[k].reshape(V, -1).float() for k in sources.ATTR_KEYS], dim=1).contiguous()
    for W in args.sizes:
        row = {}
        calls = [0]
        real = atlas._levels

        def counted(*a):
            calls[0] += 1
            return real(*a)
        atlas._levels = counted
        try:
            at, row["build_peak_mb"] = peak_mb(lambda: atlas.build(v, t, size=W))
            row["level_passes_of_the_search"] = calls[0]
        finally:
            atlas._levels = real
        row["build_ms_median_min_spread"] = host_timed(lambda: atlas.build(v, t, size=W), max(3, args.repeats // 3), warmup=1)
        level, rot, hist = torch.empty_like(at.level), torch.empty_like(at.rot), torch.zeros(16, dtype=torch.int64, device=dev)
        row["levels_ms_median_min_spread"] = host_timed(
            lambda: atlas._levels(v, t, W, at.gutter, at.lmin, at.lmax, at.density, level, rot, hist), args.repeats)
        row["sort_ms_median_min_spread"] = timed(lambda: torch.sort(at.lmax - at.level, stable=True), args.repeats)
        table = (ctypes.c_int64 * 16)(*at.counts)
        chart, uv = torch.empty_like(at.chart), torch.empty_like(at.uv)
        row["charts_ms_median_min_spread"] = timed(lambda: L.esr_atlas_charts(
            F, _lib.ptr(at.order), _lib.ptr(at.rot), table, W, at.gutter, at.lmin, at.lmax, _lib.ptr(chart), _lib.ptr(uv), st), args.repeats)
        face, bary, point, flags = (torch.empty_like(x) for x in (at.face, at.bary, at.point, at.flags))
        tex = torch.empty(W, W, 12, dtype=torch.float32, device=dev)

        def texel_pass(with_tex):
            return L.esr_atlas_texels(_lib.ptr(v), V, _lib.ptr(t), F, _lib.ptr(at.order), _lib.ptr(at.rot), table, W, at.gutter, at.lmin,
                                      at.lmax, _lib.ptr(packed) if with_tex else None, 12 if with_tex else 0, _lib.ptr(face), _lib.ptr(bary),
                                      _lib.ptr(point), _lib.ptr(flags), _lib.ptr(tex) if with_tex else None, st)
        assert texel_pass(True) == 0 and texel_pass(False) == 0
        for name, with_tex, per_texel in (("texels", False, 29), ("texels_12_channels", True, 29 + 48)):
            ms = timed(lambda: texel_pass(with_tex), args.repeats)
            rate = W * W * per_texel / (ms[0] * 1e-3) / 1e12
            row[name] = dict(ms_median_min_spread=ms, bytes_written_per_texel=per_texel, tb_per_s_written=round(rate, 3),
                             share_of_hbm_copy_rate=round(rate / res["hbm_copy_rate_tbs"], 3))
        own, inside = float((at.face >= 0).float().mean()), float((at.flags & 1).float().mean())
        row.update(density_texels_per_unit=round(at.density, 3), counts={str(l): n for l, n in enumerate(at.counts) if n},
                   share_owned=round(own, 4), share_inside=round(inside, 4))
        (textures, row["bake_model_peak_mb"]) = peak_mb(lambda: sources.bake_materials(surf, at, model=model))
        row["bake_model_ms_median_min_spread"] = timed(lambda: sources.bake_materials(surf, at, model=model), max(3, args.repeats // 3), warmup=1)
        row["bake_model_texels"] = int((at.face >= 0).sum())
        row["bake_vertices_ms_median_min_spread"] = timed(lambda: sources.bake_materials(surf, at), args.repeats)
        tex11 = torch.cat([textures[k].reshape(W, W, -1) for k in sources.TEXTURE_KEYS], dim=2).contiguous()
        row["sample_11_channels"] = dict(queries=int(hit.face.shape[0]), hits=int((hit.face >= 0).sum()),
                                         ms_median_min_spread=timed(lambda: atlas.sample(at, tex11, hit.face, hit.bary), args.repeats))
        res[f"size_{W}"] = row
        print(f"size_{W}", json.dumps(row), flush=True)
        del at, textures, tex11, tex, face, bary, point, flags
        torch.cuda.empty_cache()
    meta = km.kernel_meta(km.asm_of(os.path.join(ROOT, "esr_nerf_amd", "csrc", "atlas.hip")))
    res["kernels"] = {re.search(r"(\w+_kernel)", km.demangle(k)).group(1): dict(vgpr=m.get("vgpr"), scratch=m.get("scratch", 0), lds=m.get("lds", 0),
                                                                              waves_per_simd=m.get("occupancy"))
                      for k, m in meta.items()}
    res["clock_state_after"] = clock_state()
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
