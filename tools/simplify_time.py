"""Times of simplifying the exported surface by quadric vertex clustering (esr_nerf_amd/mesh.py: simplify, simplify_to;
csrc/simplify.hip), beside the float64 numpy restatement (tests/simplify_ref.py: fast) on a case it can finish.

    python tools/simplify_time.py [--lattice 512] [--repeats 10] [--out profiles/simplify_time.json]

Mesh: the marching-cubes surface of tools/raster_time.py (two bumpy shells on a ``--lattice``^3 lattice, 2.5 M faces at
512) with 12 attribute channels per vertex, what a ``sources.Surface`` carries.  By device events after a warm-up (median
and minimum of ``--repeats``), at cell sizes of 2, 4 and 8 lattice steps:
  faces       the clustering and the face pass: cell keys, torch.unique, face keys, two stable sorts, the keep kernel
  segments    the pair keys, their sort, the member sort and the segment offsets
  clusters    esr_simplify_clusters alone: sums, mean, solve, clip, attributes; with the bytes it has to move at least
              (pairs, triangles, each vertex and its attributes once, the outputs) and the share of the measured HBM
              copy rate (6.29 TB/s) that implies
  simplify    the whole of mesh.simplify, its read-backs of sizes included
Then ``simplify_to`` at 100 k faces (the trials counted), the sweep of ``big`` on the cluster pass at 2, 4, 8, 16 and 64 lattice
steps (at 64 a cluster holds thousands of faces), and the restatement on the host beside the device on the 64^3 surface.
The clock state is noted as far as the box lets it be read.  One JSON object, printed and written to ``--out``.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from raster_time import HBM_TBS, clock_state, surface, timed  # noqa: E402


def attributes(verts, n_c=12):
    return torch.stack([torch.sin(3.0 * verts[:, i % 3] + i) for i in range(n_c)], 1).float().contiguous()


def stages(verts, tris, attr, h, big, repeats):
    from esr_nerf_amd import mesh
    dev = verts.device

    def alloc(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=dev)

    h, origin = mesh._check_cell("simplify_time", verts, h)
    ckeys, counts, vc, keep, used = mesh._simplify_faces(verts, tris, h, origin, alloc)
    seg = mesh._simplify_segments(tris, vc, counts, alloc)
    out = {"faces": timed(lambda: mesh._simplify_faces(verts, tris, h, origin, alloc), repeats),
           "segments": timed(lambda: mesh._simplify_segments(tris, vc, counts, alloc), repeats),
           "clusters": timed(lambda: mesh._simplify_clusters(verts, tris, attr, vc, ckeys, seg, origin, h, 1e-3, big, False, alloc),
                             repeats),
           "simplify": timed(lambda: mesh.simplify(verts, tris, h, attr=attr, big=big), repeats)}
    n_v, n_f, n_k, n_c = int(verts.shape[0]), int(tris.shape[0]), int(ckeys.shape[0]), int(attr.shape[1])
    n_pairs = int(seg[2][-1])
    per = (seg[2][1:] - seg[2][:-1])
    need = 8 * n_pairs + 24 * n_f + (24 + 4 + 4 * n_c + 8) * n_v + (8 + 16 + 24 + 4 * n_c) * n_k
    return dict(cell=h, clusters=n_k, kept_faces=int(keep.sum()), kept_vertices=int(used.sum()), pairs=n_pairs,
                largest_cluster_pairs=int(per.max()), clusters_over_big=int((per > big).sum()), ms_median_min=out,
                clusters_bytes_needed=need,
                clusters_share_of_hbm_copy_rate=round(need / (out["clusters"][0] * 1e-3) / (HBM_TBS * 1e12), 4))


def big_sweep(verts, tris, attr, h, repeats):
    from esr_nerf_amd import mesh
    dev = verts.device

    def alloc(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=dev)

    h, origin = mesh._check_cell("simplify_time", verts, h)
    ckeys, counts, vc, _, _ = mesh._simplify_faces(verts, tris, h, origin, alloc)
    seg = mesh._simplify_segments(tris, vc, counts, alloc)
    per = torch.maximum(seg[2][1:] - seg[2][:-1], counts)
    by = {}
    for big in (16, 32, 64, 128, 256, 1024, 1 << 30):
        ms = timed(lambda: mesh._simplify_clusters(verts, tris, attr, vc, ckeys, seg, origin, h, 1e-3, big, False, alloc), repeats)
        by[str(big)] = dict(clusters_ms=ms, on_the_workgroup_path=int((per > big).sum()))
    return dict(cell=h, clusters=int(ckeys.shape[0]), largest_cluster=int(per.max()), by_big=by)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--target", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("simplify_time.py measures on the GPU; none is visible")
    from esr_nerf_amd import mesh
    import simplify_ref as sr
    dev = torch.device("cuda:0")
    step = 2.0 / (args.lattice - 1)
    res = dict(lattice=args.lattice, repeats=args.repeats, device=torch.cuda.get_device_name(0), default_big=mesh.SIMPLIFY_BIG,
               hbm_copy_rate_tbs=HBM_TBS, clock_state_before=clock_state())
    verts, tris = surface(args.lattice, dev)
    attr = attributes(verts)
    res.update(vertices=int(verts.shape[0]), faces=int(tris.shape[0]), attr_channels=int(attr.shape[1]))
    res["by_cell_in_lattice_steps"] = {str(c): stages(verts, tris, attr, c * step, mesh.SIMPLIFY_BIG, args.repeats) for c in (2, 4, 8)}

    trials = [0]
    inner = mesh._simplify_faces

    def counted(*a):
        trials[0] += 1
        return inner(*a)

    mesh._simplify_faces = counted
    try:
        state = {}

        def to():
            trials[0] = 0
            state["out"] = mesh.simplify_to(verts, tris, args.target, attr=attr)

        ms = timed(to, max(3, args.repeats // 3), warmup=1)
    finally:
        mesh._simplify_faces = inner
    out, cell, over = state["out"]
    res["simplify_to"] = dict(target_faces=args.target, faces=int(out[1].shape[0]), cell=cell, cell_over=over,
                              cell_in_lattice_steps=round(cell / step, 3), face_passes=trials[0], ms_median_min=ms)
    res["big_sweep_by_cell_in_lattice_steps"] = {str(c): big_sweep(verts, tris, attr, c * step, args.repeats) for c in (2, 4, 8, 16, 64)}

    # the restatement on the host beside the device, on a case numpy finishes: the 64^3 surface at 4 lattice steps
    cv, ct = surface(64, dev)
    ca = attributes(cv)
    ch = 4 * 2.0 / 63
    hv, ht, ha = cv.cpu().numpy(), ct.cpu().numpy(), ca.cpu().numpy()
    t0 = time.perf_counter()
    ref = sr.fast(hv, ht, ch, 1e-3, ha)
    tri_ref, _, new_id = sr.faces(ref["vc"], ht, len(ref["keys"]))
    host_ms = (time.perf_counter() - t0) * 1e3
    dev_ms = timed(lambda: mesh.simplify(cv, ct, ch, attr=ca), args.repeats)
    got = mesh.simplify(cv, ct, ch, attr=ca)
    same = bool(np.array_equal(got[1].cpu().numpy(), tri_ref))
    worst = float(np.abs(got[0].cpu().numpy() - ref["pos"][new_id >= 0]).max())
    res["restatement_on_the_host"] = dict(lattice=64, faces=int(ct.shape[0]), kept_faces=int(len(tri_ref)), cell=ch,
                                          numpy_float64_form_and_python_face_rules_ms=round(host_ms, 1),
                                          device_simplify_ms_median_min=dev_ms, triangles_equal=same,
                                          worst_position_difference=worst,
                                          what="tests/simplify_ref.py fast() + faces(), one run by the host clock")
    res["clock_state_after"] = clock_state()
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
