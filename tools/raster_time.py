"""Pass times of rasterising the exported surface into 800 x 800 views (esr_nerf_amd/raster.py, csrc/raster.hip), beside the
only other route to a view's emission mask: a volumetric render of the view and ``any(x > k_val)`` on it.

    python tools/raster_time.py [--size 800] [--lattice 512] [--views 100] [--repeats 20] [--out profiles/raster_time.json]

Mesh: the marching-cubes surface of a ``--lattice``^3 analytic field (two bumpy shells), millions of faces that cover about
a pixel each.  Per view, by device events after a warm-up (median and minimum of ``--repeats``):
  faces_small    esr_raster_faces with big_px so large that no face is queued: clear + the per-(view, face) pass (+ the
                 launch of the large-face kernel on an empty queue)
  faces          the same call with the default big_px; ``large`` = faces - faces_small
  resolve, masks esr_raster_resolve; esr_source_masks with two conditions
and the bytes each pass has to move at least, with the share of the measured HBM copy rate (6.29 TB/s) that implies.
Then ``--views`` views through ``raster.rasterize`` in its chunks (per view), a sweep of big_px on a coarse (64^3) surface of
the same field, whose faces cover ~100 pixels each, and the parent route: ``evaluate.render_view`` of VoxurfF on the C2 slab
scene (the model of tools/eval_time.py) + the threshold.  The clock state is noted as far as the box lets it be read.
One JSON object, printed and written to ``--out``.
"""
import argparse
import ctypes as C
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_TBS = 6.29                                       # measured float4 copy rate of the MI355X


def timed(fn, repeats, warmup=3):
    """(median, min) milliseconds of fn() by device events"""
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
    return round(float(np.median(ms)), 4), round(float(np.min(ms)), 4)


def clock_state():
    out = {}
    for p in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"))[:1]:
        try:
            out["pp_dpm_sclk"] = [l.strip() for l in open(p).read().splitlines()]
        except OSError as e:
            out["pp_dpm_sclk"] = f"unreadable: {e}"
    try:
        out["torch_clock_rate_mhz"] = int(torch.cuda.clock_rate(0))
    except Exception as e:                           # (needs the management library's Python binding)
        out["torch_clock_rate_mhz"] = f"unavailable: {type(e).__name__}"
    return out or "not readable on this box"


def field(n, dev):
    """positive between two bumpy shells: an outer and an inner surface"""
    ax = torch.linspace(-1, 1, n, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    r = torch.sqrt(x * x + y * y + z * z)
    bump = 0.06 * torch.sin(9 * x) * torch.cos(7 * y) * torch.sin(8 * z + 0.3)
    return torch.minimum(0.86 + bump - r, r - 0.5 + 0.5 * bump).float().contiguous()


def surface(n, dev):
    from esr_nerf_amd import mesh
    v, t = mesh.marching_cubes(field(n, dev), 0.0)
    return (v / (n - 1) * 2.0 - 1.0).contiguous(), t


def ring_cameras(n_views, size, dev):
    from esr_nerf_amd.camera import Cameras
    poses = []
    for k in range(n_views):
        a = 2 * np.pi * k / n_views
        eye = np.array([3.0 * np.cos(a), 3.0 * np.sin(a), 0.8 * np.sin(3 * a)])
        z = -eye / np.linalg.norm(eye)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        poses.append(np.concatenate([np.stack([x, np.cross(z, x), z], 1), eye[:, None]], 1))
    return Cameras(torch.from_numpy(np.stack(poses).astype(np.float32)).to(dev), 1.35 * size, 1.35 * size, size / 2, size / 2, size, size)


def passes(verts, tris, cams, face_source, n_src, big_px, repeats):
    """per-view pass times through the C ABI on view 0"""
    from esr_nerf_amd import _lib, raster
    L, dev = _lib.lib(), verts.device
    s = _lib.stream_ptr(dev)
    n_f, n_v, n_px = int(tris.shape[0]), int(verts.shape[0]), cams.width * cams.height
    cam = cams.struct()
    w2c = torch.from_numpy(raster.world_to_camera(cams)).to(dev)
    zbuf = torch.empty(n_px, dtype=torch.int64, device=dev)
    queue = torch.empty(n_f, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    drop = torch.empty(1, dtype=torch.int32, device=dev)
    face = torch.empty(n_px, dtype=torch.int32, device=dev)
    depth = torch.empty(n_px, dtype=torch.float32, device=dev)
    cond = torch.from_numpy(raster._conditions(n_src, [list(range(0, n_src, 2)), list(range(1, n_src, 2))])).to(dev)
    masks = torch.empty(2 * n_px, dtype=torch.float32, device=dev)
    pixels = torch.empty(max(n_src, 1), dtype=torch.int64, device=dev)

    def faces(big):
        _lib.check(L.esr_raster_faces(C.byref(cam), _lib.ptr(w2c), 0, 1, _lib.ptr(verts), n_v, _lib.ptr(tris), n_f, raster.Z_NEAR,
                                      big, _lib.ptr(zbuf), _lib.ptr(drop), _lib.ptr(queue), n_f, _lib.ptr(count), s), "faces")

    out = {"faces_small": timed(lambda: faces(1 << 40), repeats), "faces": timed(lambda: faces(big_px), repeats)}
    queued = int(count.item())
    out["resolve"] = timed(lambda: _lib.check(L.esr_raster_resolve(_lib.ptr(zbuf), n_px, _lib.ptr(face), _lib.ptr(depth), s),
                                              "resolve"), repeats)
    out["masks"] = timed(lambda: _lib.check(L.esr_source_masks(_lib.ptr(face), 1, n_px, _lib.ptr(face_source), n_f, _lib.ptr(cond),
                                                               n_src, 2, _lib.ptr(masks), _lib.ptr(pixels), s), "masks"), repeats)
    covered = int((face >= 0).sum())
    # what each pass has to move at least: indices and (each vertex once) coordinates in, one word per pixel cleared and
    # one read-modify-write per covered pixel; words in, face + depth out; faces in, source ids gathered, masks out
    need = {"faces_small": 24 * n_f + 24 * n_v + 8 * n_px + 16 * covered, "resolve": 16 * n_px,
            "masks": 4 * n_px + 4 * covered + 2 * 4 * n_px}
    share = {k: round(need[k] / (out[k][0] * 1e-3) / (HBM_TBS * 1e12), 4) for k in need}
    return dict(ms_median_min=out, large_ms=round(out["faces"][0] - out["faces_small"][0], 4), queued_faces=queued,
                covered_pixels=covered, dropped=int(drop.item()), bytes_needed=need, share_of_hbm_copy_rate=share)


def parent_route(size, batch, k_val=0.5):
    """render_view of VoxurfF on the C2 slab scene (tools/eval_time.py's model) and the mask any(x > k_val) of a colour key"""
    from esr_nerf_amd import evaluate
    from esr_nerf_amd.config import fine_cfg
    from esr_nerf_amd.synthetic import init_slab_model, slab_scene
    from esr_nerf_amd.voxurff import VoxurfF
    sc = slab_scene("C2", s_val=60.0, oblique=True, n_rays=size * size)
    torch.manual_seed(0)
    np.random.seed(0)
    m = VoxurfF(fine_cfg("cuda:0"), sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max,
                sc.mask_alpha_init, sc.mask_density, sc.s_val, sc.num_voxels)
    init_slab_model(m, sc)
    m.s_val = sc.s_val
    m.eval()
    b = {k: sc.batch[k].cuda() for k in ("rays_o", "rays_d", "viewdirs")}
    pos = torch.eye(3).cuda()
    state = {}

    def route():
        raw = evaluate.render_view(m, b["rays_o"], b["rays_d"], b["viewdirs"], 1, pos, size, size, batch)
        key = "lin/emit" if "lin/emit" in raw else next(k for k, x in raw.items() if x.dim() == 3 and x.shape[-1] == 3)
        state["key"], state["mask"] = key, (raw[key] > k_val).any(-1)

    ms = timed(route, 3, warmup=1)
    return dict(ms_median_min=ms, thresholded_key=state["key"], batch=batch, model="VoxurfF on slab_scene('C2')")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--lattice", type=int, default=512)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--no-parent", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("raster_time.py measures on the GPU; none is visible")
    from esr_nerf_amd import raster
    dev = torch.device("cuda:0")
    res = dict(size=args.size, lattice=args.lattice, repeats=args.repeats, device=torch.cuda.get_device_name(0),
               default_big_px=raster.BIG_PX, hbm_copy_rate_tbs=HBM_TBS, clock_state_before=clock_state())
    verts, tris = surface(args.lattice, dev)
    n_f, n_src = int(tris.shape[0]), 8
    res.update(vertices=int(verts.shape[0]), faces=n_f)
    face_source = (torch.arange(n_f, device=dev) * n_src // max(n_f, 1)).to(torch.int32)       # 8 sources of contiguous faces
    face_source[::5] = -1
    cams = ring_cameras(args.views, args.size, dev)
    res["one_view"] = passes(verts, tris, cams, face_source, n_src, raster.BIG_PX, args.repeats)

    def many():
        r = raster.rasterize(verts, tris, cams)
        raster.source_masks(r.face, face_source, n_src, [[0, 2, 4, 6], [1, 3, 5, 7]])

    per_view = 8 * (args.size * args.size + n_f)
    ms = timed(many, 3, warmup=1)
    res["many_views"] = dict(views=args.views, views_per_chunk=max(1, raster.CHUNK_BYTES // per_view),
                             total_ms_median_min=ms, per_view_ms=round(ms[0] / args.views, 4),
                             what="raster.rasterize (chunked) + raster.source_masks, two conditions")
    # big_px: a coarse surface of the same field, whose faces cover ~100 pixels each
    cv, ct = surface(64, dev)
    cs = torch.zeros(int(ct.shape[0]), dtype=torch.int32, device=dev)
    sweep = {}
    for big in (0, 4, 16, 64, 256, 1024, 1 << 30):
        p = passes(cv, ct, cams, cs, 1, big, args.repeats)
        sweep[str(big)] = dict(faces_ms=p["ms_median_min"]["faces"], queued_faces=p["queued_faces"])
    res["big_px_sweep_coarse_surface"] = dict(lattice=64, faces=int(ct.shape[0]), by_big_px=sweep)
    sweep = {}
    for big in (0, 4, 16, 64, 256, 1 << 30):
        p = passes(verts, tris, cams, face_source, n_src, big, max(3, args.repeats // 4))
        sweep[str(big)] = dict(faces_ms=p["ms_median_min"]["faces"], queued_faces=p["queued_faces"])
    res["big_px_sweep_fine_surface"] = dict(lattice=args.lattice, faces=n_f, by_big_px=sweep)
    if not args.no_parent:
        res["parent_route_render_and_threshold"] = parent_route(args.size, args.batch)
    res["clock_state_after"] = clock_state()
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
