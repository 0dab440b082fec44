"""Device-event times of the surface export (esr_nerf_amd/sources.py, mesh.py) beside the host body it replaces.

    python tools/surface_time.py [--config C4] [--resolution 512] [--repeats 5] [--out profiles/surface_time.json]

On the resolution^3 surface of a BASELINE config's analytic SDF (synthetic.slab_scene / init_slab_model; the light-transport
model, so that the material heads exist): median milliseconds of
  field_mc      mesh.sdf_field + mesh.marching_cubes
  attributes    ESRNeRF.surface_attributes at every vertex
  components    mesh.connected_components (link, flatten, the rank scan, labels) of the whole mesh
  stats         mesh.component_stats with the emission as attribute: the in-wave reduction, and ``stats_per_lane``: one
                atomic per face and quantity (on a mesh that is ONE component: every atomic on one slot)
  sources       emissive_sources at the median emission (mask, components, statistics)
and, timed on the same machine with the host's clock, what a user of the reference would run on the same mesh:
  host_copy     vertices, triangles and emission to numpy
  host_scipy    scipy.sparse.csgraph.connected_components on the vertex graph + face labels
  host_sums     numpy: face areas, np.bincount sums of area / centroid / emission per component, np.minimum.at boxes
One JSON document goes to --out and to stdout.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from esr_nerf_amd import mesh  # noqa: E402
from esr_nerf_amd.sources import Surface, emissive_sources  # noqa: E402


def build_model(config, dev):
    from esr_nerf_amd.config import lts_cfg
    from esr_nerf_amd.esrnerf import ESRNeRF
    from esr_nerf_amd.synthetic import init_slab_model, slab_scene
    sc = slab_scene(config, s_val=20.0)
    torch.manual_seed(0)
    np.random.seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = ESRNeRF(lts_cfg(dev), sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max,
                    sc.mask_alpha_init, sc.mask_density, sc.s_val, sc.num_voxels)
    init_slab_model(m, sc)
    with torch.no_grad():
        m.brdf.grid.normal_(0.0, 0.1)
    m.s_val = 20.0
    m.eval()
    return m


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def host_components(t, n_v):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    i = np.concatenate([t[:, 0], t[:, 0], t[:, 1]])
    j = np.concatenate([t[:, 1], t[:, 2], t[:, 2]])
    k, vlab = connected_components(coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n_v, n_v)), directed=False)
    return vlab[t[:, 0]], k


def host_sums(v, t, em, lab, k):
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    out = [np.bincount(lab, minlength=k), np.bincount(lab, area, k)]
    cen = area[:, None] * (a + b + c) / 3.0
    fem = area[:, None] * (em[t[:, 0]].astype(np.float64) + em[t[:, 1]] + em[t[:, 2]]) / 3.0
    out += [np.stack([np.bincount(lab, x[:, d], k) for d in range(3)], 1) for x in (cen, fem)]
    lo, hi = np.full((k, 3), np.inf), np.full((k, 3), -np.inf)
    np.minimum.at(lo, lab, np.minimum(np.minimum(a, b), c))
    np.maximum.at(hi, lab, np.maximum(np.maximum(a, b), c))
    return out + [lo, hi]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_time.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = build_model(args.config, dev)
    R = args.resolution
    lo, hi = (b.to(dev) for b in mesh._box(model))

    def field_mc():
        u = mesh.sdf_field(model, R)
        v, t = mesh.marching_cubes(u, 0.0)
        return (v / (R - 1.0) * (hi - lo).double() + lo.double()).contiguous(), t

    stages = {k: [] for k in ("field_mc", "attributes", "components", "stats", "stats_per_lane", "sources", "host_copy",
                              "host_scipy", "host_sums")}
    info = {}
    for rep in range(args.repeats + 1):              # the first pass warms up and is dropped
        (v, t), ms = device_ms(field_mc)
        stages["field_mc"].append(ms)
        pts = torch.minimum(torch.maximum(v.float(), lo), hi)
        attrs, ms = device_ms(lambda: model.surface_attributes(pts))
        stages["attributes"].append(ms)
        (lab, k), ms = device_ms(lambda: mesh.connected_components(t, v.shape[0]))
        stages["components"].append(ms)
        em = attrs["emission"]
        st, ms = device_ms(lambda: mesh.component_stats(v, t, lab, k, em))
        stages["stats"].append(ms)
        st2, ms = device_ms(lambda: mesh.component_stats(v, t, lab, k, em, per_lane_atomics=True))
        stages["stats_per_lane"].append(ms)
        k_val = float(em.max(dim=1).values.median())
        rep_, ms = device_ms(lambda: emissive_sources(Surface(v, t, attrs), k_val))
        stages["sources"].append(ms)
        (hv, ht, hem), ms = host_ms(lambda: (v.cpu().numpy(), t.cpu().numpy(), em.cpu().numpy()))
        stages["host_copy"].append(ms)
        (hlab, hk), ms = host_ms(lambda: host_components(ht, len(hv)))
        stages["host_scipy"].append(ms)
        hs, ms = host_ms(lambda: host_sums(hv, ht, hem, hlab, hk))
        stages["host_sums"].append(ms)
        assert hk - (len(hv) - len(np.unique(ht))) == k
        assert np.array_equal(np.sort(hs[0][hs[0] > 0]), np.sort(st["n_faces"].cpu().numpy()))
        assert abs(float(st["area"].sum()) - float(hs[1].sum())) <= 1e-9 * float(hs[1].sum())
        assert torch.equal(st["n_faces"], st2["n_faces"]) and torch.equal(st["bbox_min"], st2["bbox_min"])
        info = dict(vertices=int(v.shape[0]), triangles=int(t.shape[0]), components=int(k), sources=len(rep_))
    med = {k: round(float(np.median(x[1:])), 3) for k, x in stages.items()}
    device_total = med["components"] + med["stats"]
    host_total = med["host_copy"] + med["host_scipy"] + med["host_sums"]
    doc = dict(config=args.config, resolution=R, repeats=args.repeats, **info, ms=med,
               device_components_plus_stats_ms=round(device_total, 3), host_body_ms=round(host_total, 3),
               host_over_device=round(host_total / device_total, 1),
               stats_per_lane_over_prereduced=round(med["stats_per_lane"] / med["stats"], 2),
               device=torch.cuda.get_device_name(dev))
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
