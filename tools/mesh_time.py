"""Device-event times of mesh export (esr_nerf_amd/mesh.py) against the torch field loop it replaces.

    python tools/mesh_time.py [--repeats N]

One JSON line per lattice resolution R (256, 512) on the 256^3 analytic-SDF grid (synthetic.analytic_sdf over the cube
[-1, 1]^3): median milliseconds of gauss (esr_gauss3d_fwd), field (esr_mesh_field), count (esr_mesh_count), scan
(torch cumsum of the block totals and the read-back of V, F), emit (esr_mesh_emit: vertices + triangles), their sum, and
torch_field (today's modules.extract_sdf_field: Gaussian3DConv + 64^3-point grid_sample blocks), after a warm-up.
"""
import argparse
import ctypes as C
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from esr_nerf_amd import _lib, mesh  # noqa: E402
from esr_nerf_amd.modules import extract_sdf_field  # noqa: E402
from esr_nerf_amd.synthetic import analytic_sdf  # noqa: E402


def timed(fn, events):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    events.append((a, b))
    return out


def one_run(model, R, thr=0.0):
    """the stages of mesh.extract_geometry's device half, each between two events"""
    L, dev = _lib.lib(), model.sdf.grid.device
    s = _lib.stream_ptr(dev)
    ev = []
    g = model.sdf.grid.detach()[0, 0].contiguous()
    sm = timed(lambda: mesh.smooth_grid(g, 0.5), ev)
    lo, hi = model.xyz_min.float().cpu(), model.xyz_max.float().cpu()
    axes = mesh.lattice_axes(lo, hi, R, dev)
    u = timed(lambda: mesh.field(sm, lo, hi, axes), ev)
    dims = list(u.shape)
    nb = int(L.esr_mesh_blocks(*dims))
    counts = torch.empty(2 * nb, dtype=torch.int64, device=dev)
    timed(lambda: _lib.check(L.esr_mesh_count(_lib.ptr(u), *dims, C.c_float(thr), _lib.ptr(counts), s), "count"), ev)
    offsets, n_v, n_f = timed(lambda: mesh._scan(counts, nb), ev)
    vid = torch.empty(dims, dtype=torch.int32, device=dev)
    verts = torch.empty(n_v, 3, dtype=torch.float64, device=dev)
    tris = torch.empty(n_f, 3, dtype=torch.int64, device=dev)
    timed(lambda: _lib.check(L.esr_mesh_emit(_lib.ptr(u), *dims, C.c_float(thr), _lib.ptr(offsets), _lib.ptr(vid),
                                             _lib.ptr(verts), _lib.ptr(tris), s), "emit"), ev)
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev], n_v, n_f


def torch_field(model, R):
    ev = []
    timed(lambda: extract_sdf_field(model, R, 64, True, 0.5), ev)
    torch.cuda.synchronize()
    return ev[0][0].elapsed_time(ev[0][1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lo, hi = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
    ws = [256, 256, 256]
    model = SimpleNamespace(xyz_min=lo.to(dev), xyz_max=hi.to(dev), world_size=torch.tensor(ws),
                            sdf=SimpleNamespace(grid=analytic_sdf(ws, lo, hi).to(dev)))
    names = ("gauss", "field", "count", "scan", "emit")
    for R in (256, 512):
        for _ in range(2):
            one_run(model, R)
            torch_field(model, R)
        runs = [one_run(model, R) for _ in range(args.repeats)]
        t = np.array([r[0] for r in runs])
        med = {n: round(float(np.median(t[:, i])), 3) for i, n in enumerate(names)}
        med["total"] = round(float(np.median(t.sum(1))), 3)
        tf = [torch_field(model, R) for _ in range(max(2, args.repeats // 2))]
        print(json.dumps(dict(R=R, grid=ws, vertices=runs[0][1], triangles=runs[0][2], repeats=args.repeats,
                              ms=med, torch_field_ms=round(float(np.median(tf)), 3),
                              device=torch.cuda.get_device_name(dev))), flush=True)


if __name__ == "__main__":
    main()
