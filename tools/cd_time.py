"""Device-event times of the DTU Chamfer metric (esr_nerf_amd/chamfer.py) on a DTU-scale synthetic case.

    python tools/cd_time.py [--repeats N] [--host]

The case (``dtu_case``): a bumpy-sphere analytic SDF extracted by mesh.marching_cubes at R = 512 and scaled to a
400 mm box; an stl cloud of 2.7 M area-weighted surface points jittered by 0.05 mm plus 0.3 M far outliers in a 1.2 m
box; an ObsMask of 2 mm voxels with a slab and random blocks unobserved; a ground plane at z = -100 mm.

One JSON line: the point counts, the downsample's rounds, and the median milliseconds (CUDA events, after a warm-up) of
sample (count + cumsum + fill), shuffle (seeded randperm + gather), downsample (cell index + rounds), filters (bounds,
ObsMask, plane), d2s and s2d (cell index over the targets + the search), and their total.  ``--host``: one more line
per stage as it ends, then their sum, with the wall-clock seconds of the numpy / sklearn restatement of the same case
(the reference's pool sampling, kd-tree radius_neighbors + keep loop, two kneighbors passes) on 16 host workers.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from esr_nerf_amd import chamfer, mesh  # noqa: E402

THRESH, MAX_DIST, PATCH = 0.2, 20.0, 60


@torch.no_grad()
def dtu_case(R=512, n_surface=2_700_000, n_far=300_000, seed=0, device="cuda:0"):
    dev = torch.device(device)
    ax = torch.linspace(-1.0, 1.0, R, device=dev)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    sdf = (X * X + Y * Y + Z * Z).sqrt() - 0.6 - 0.04 * torch.sin(7 * X) * torch.sin(5 * Y) * torch.sin(6 * Z)
    u = (-sdf).float().contiguous()
    del X, Y, Z, sdf
    v, f = mesh.marching_cubes(u, 0.0)
    del u
    v = (v / (R - 1) * 2.0 - 1.0) * 200.0                    # a 400 mm box, as a DTU scan
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    tv = v[f]
    area = torch.linalg.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]).norm(dim=1)
    pick = torch.multinomial(area.float(), n_surface, replacement=True, generator=g)
    a, b = torch.rand(n_surface, 1, generator=g, device=dev, dtype=torch.float64), \
        torch.rand(n_surface, 1, generator=g, device=dev, dtype=torch.float64)
    flip = (a + b) > 1
    a, b = torch.where(flip, 1 - a, a), torch.where(flip, 1 - b, b)
    t = tv[pick]
    surf = t[:, 0] + a * (t[:, 1] - t[:, 0]) + b * (t[:, 2] - t[:, 0])
    surf += 0.05 * torch.randn(surf.shape, generator=g, device=dev, dtype=torch.float64)
    far = (torch.rand(n_far, 3, generator=g, device=dev, dtype=torch.float64) - 0.5) * 1200.0
    stl = torch.cat([surf, far]).cpu().numpy()
    res = 2.0
    bb = np.array([[-230.0, -230.0, -230.0], [230.0, 230.0, 230.0]])
    shape = tuple(int(math.floor((bb[1, a] - bb[0, a]) / res)) + 1 for a in range(3))
    rng = np.random.default_rng(seed)
    obs = np.ones(shape, bool)
    obs[:, 150:165, :] = False
    for _ in range(40):
        c = rng.integers(0, np.array(shape) - 12)
        obs[c[0]:c[0] + 12, c[1]:c[1] + 12, c[2]:c[2] + 12] = False
    plane = np.array([0.0, 0.0, 1.0, 100.0])
    return dict(vertices=v, triangles=f, obs_mask=obs, bb=bb, res=np.array([[res]]), stl=stl, plane=plane)


def run_stages(c, seed=0):
    """dtu_chamfer's stages, each between two events -> (ms per stage, stats, means)"""
    ev, st = [], {}

    def timed(name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        ev.append((name, a, b))
        return out

    dev = c["vertices"].device
    pts = timed("sample", lambda: chamfer.sample_mesh_points(c["vertices"], c["triangles"], THRESH))
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    data = timed("shuffle", lambda: pts[torch.randperm(pts.shape[0], generator=g, device=dev)].contiguous())
    keep, rounds = timed("downsample", lambda: chamfer.radius_downsample(data, THRESH, return_rounds=True))
    stl = torch.as_tensor(c["stl"], device=dev)

    def filt():
        data_in, data_in_obs = chamfer.dtu_filters(data[keep], c["obs_mask"], c["bb"], c["res"], PATCH)
        return data_in, data_in_obs, stl[chamfer.above_plane(stl, c["plane"])].contiguous()

    data_in, data_in_obs, stl_above = timed("filters", filt)
    d2s = timed("d2s", lambda: chamfer.nn_distance(data_in_obs, stl, MAX_DIST))
    s2d = timed("s2d", lambda: chamfer.nn_distance(stl_above, data_in, MAX_DIST))
    torch.cuda.synchronize()
    ms = {n: a.elapsed_time(b) for n, a, b in ev}
    st.update(points=int(pts.shape[0]), kept=int(keep.sum()), data_in=int(data_in.shape[0]),
              data_in_obs=int(data_in_obs.shape[0]), stl=int(stl.shape[0]), stl_above=int(stl_above.shape[0]),
              rounds=rounds)
    means = (chamfer._mean_below(d2s, MAX_DIST), chamfer._mean_below(s2d, MAX_DIST))
    return ms, st, means


def _host_tri(args):
    n1, n2, v1, v2, p0 = args
    i, j = np.meshgrid(np.arange(n1 + 1), np.arange(n2 + 1), indexing="ij")
    a = (i.reshape(-1) + 0.5) / max(n1, 1e-7)
    b = (j.reshape(-1) + 0.5) / max(n2, 1e-7)
    k = a + b < 1
    return v1 * a[k, None] + v2 * b[k, None] + p0


def host_times(c, workers=16):
    """the numpy / sklearn restatement of the same case, wall-clock seconds per stage"""
    import multiprocessing as mp

    import sklearn.neighbors as skln
    out = {}

    def done(name, t0):
        out[name] = round(time.perf_counter() - t0, 2)
        print(json.dumps(dict(host_stage=name, s=out[name])), flush=True)

    t0 = time.perf_counter()
    v, f = c["vertices"].cpu().numpy(), c["triangles"].cpu().numpy()
    tv = v[f]
    v1, v2 = tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]
    l1, l2 = np.linalg.norm(v1, axis=-1), np.linalg.norm(v2, axis=-1)
    area2 = np.linalg.norm(np.cross(v1, v2), axis=-1)
    nz = area2 > 0
    thr = THRESH * np.sqrt(l1[nz] * l2[nz] / area2[nz])
    n1, n2 = np.floor(l1[nz] / thr), np.floor(l2[nz] / thr)
    v1, v2, p0 = v1[nz], v2[nz], tv[nz, 0]
    with mp.Pool(workers) as pool:
        parts = pool.map(_host_tri, ((n1[i], n2[i], v1[i], v2[i], p0[i]) for i in range(len(n1))), chunksize=1024)
    data = np.concatenate([v] + parts)
    np.random.default_rng(0).shuffle(data, axis=0)
    done("sample_shuffle", t0)
    t0 = time.perf_counter()
    eng = skln.NearestNeighbors(n_neighbors=1, radius=THRESH, algorithm="kd_tree", n_jobs=workers).fit(data)
    idxs = eng.radius_neighbors(data, radius=THRESH, return_distance=False)
    mask = np.ones(len(data), bool)
    for cur, ids in enumerate(idxs):
        if mask[cur]:
            mask[ids] = 0
            mask[cur] = 1
    del idxs
    done("downsample", t0)
    t0 = time.perf_counter()
    down = data[mask]
    eng.fit(c["stl"])
    eng.kneighbors(down, n_neighbors=1, return_distance=True)
    done("d2s", t0)
    t0 = time.perf_counter()
    above = c["stl"][(c["stl"] @ c["plane"][:3]) + c["plane"][3] > 0]
    eng.fit(down)
    eng.kneighbors(above, n_neighbors=1, return_distance=True)
    done("s2d", t0)
    out["total"] = round(sum(out.values()), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    c = dtu_case(device=dev)
    run_stages(c)
    runs = [run_stages(c) for _ in range(args.repeats)]
    names = list(runs[0][0])
    ms = {n: round(float(np.median([r[0][n] for r in runs])), 2) for n in names}
    ms["total"] = round(float(np.median([sum(r[0].values()) for r in runs])), 2)
    print(json.dumps(dict(vertices=int(c["vertices"].shape[0]), triangles=int(c["triangles"].shape[0]), **runs[0][1],
                          repeats=args.repeats, ms=ms, mean_d2s=runs[0][2][0], mean_s2d=runs[0][2][1],
                          device=torch.cuda.get_device_name(dev))), flush=True)
    if args.host:
        print(json.dumps(dict(host_s=host_times(c), workers=16)), flush=True)


if __name__ == "__main__":
    main()
