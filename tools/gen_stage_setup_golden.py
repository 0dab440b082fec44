"""Write tests/golden/stage_setup.npz: the reference's own stage hand-over on small grids, on CPU.

    python tools/gen_stage_setup_golden.py            (CPU host with the reference tree)

The reference classes are loaded by path the way tools/gen_dvgo_golden.py loads DVGO (``omegaconf`` stubbed; for
app/utils/base/module.py also ``app.utils.base.functions``, whose CUDA extensions none of the methods used here touches):
``DVGO.grid_sampler``, ``DVGO.activate_density``, ``MaskCache`` and ``DenseGrid.scale_volume_grid``.  The few trainer lines
around them (coarse.py:152-187: the node coordinates, the threshold, amin / amax, the widening; voxurff.py:571-593: the
grid's node coordinates) are written afresh here.  Inputs come from tests/setup_ref64.py, so the tests can rebuild them.

Recorded:  ``am/*``     an alphamask record (19 x 16 x 12 density with a blob, its box, alpha_init, near, far), the bounding
                        box of its active nodes at bbox_thres, the count, and the box widened by world_bound_scale
           ``mc/*``     MaskCache of that density (ks 3): the pooled density and its decision at the nodes of a 19 x 16 x 12
                        and a 2 x 1 x 3 grid whose boxes lie inside and reach outside the mask box
           ``up/*``     DenseGrid.scale_volume_grid (5,7,3) -> (13,9,4) with 1 and 6 channels
The tests only read the .npz.
"""
import importlib.util
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF_ROOT = os.environ.get("ESR_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "stage_setup.npz")

NEAR, FAR, NUM_VOXELS, BBOX_THRES, WORLD_BOUND_SCALE, MASK_KS = 0.2, 6.0, 4000, 1e-3, 1.05, 3


def by_path(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF_ROOT, *rel.split("/")))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    om = types.ModuleType("omegaconf")
    om.DictConfig = type("DictConfig", (dict,), {})
    sys.modules.setdefault("omegaconf", om)
    for name in ("app", "app.utils", "app.utils.base"):
        sys.modules.setdefault(name, types.ModuleType(name))
    fn = types.ModuleType("app.utils.base.functions")
    fn.render_utils_cuda = fn.total_variation_cuda = None
    sys.modules.setdefault("app.utils.base.functions", fn)
    return by_path("ref_dvgo", "app/coarse/model/dvgo.py").DVGO, by_path("ref_module", "app/utils/base/module.py")


def main():
    import setup_ref64 as R
    DVGO, module = load_reference()
    lo, hi = torch.tensor(R.MASK_BOX[:3]), torch.tensor(R.MASK_BOX[3:])
    cfg = SimpleNamespace(system=SimpleNamespace(device="cpu"),
                          app=SimpleNamespace(model=SimpleNamespace(num_voxels=NUM_VOXELS, stepsize=0.5, alpha_init=R.ALPHA_INIT)))
    am = DVGO(cfg, NEAR, FAR, lo, hi)
    density = torch.from_numpy(R.bounds_density("blob-19x16x12"))[None, None]
    assert tuple(am.density.shape) == tuple(density.shape), am.density.shape
    with torch.no_grad():
        am.density.copy_(density)
    out = dict(**{"am/xyz_min": lo.numpy(), "am/xyz_max": hi.numpy(), "am/near": np.float64(NEAR), "am/far": np.float64(FAR),
                  "am/alpha_init": np.float64(R.ALPHA_INIT), "am/density": density.numpy(),
                  "am/bbox_thres": np.float64(BBOX_THRES), "am/world_bound_scale": np.float64(WORLD_BOUND_SCALE)})

    # compute_bbox_by_coarse_geo
    with torch.no_grad():
        t = [torch.linspace(0, 1, n) for n in density.shape[2:]]
        interp = torch.stack(torch.meshgrid(*t, indexing="ij"), -1)
        nodes = lo * (1 - interp) + hi * interp
        alpha = am.activate_density(am.grid_sampler(nodes, am.density))
        active = nodes[alpha > BBOX_THRES]
        bmin, bmax = active.amin(0), active.amax(0)
        out.update({"am/active": np.int64(len(active)), "am/bbox_min": bmin.numpy(), "am/bbox_max": bmax.numpy()})
        shift = (bmax - bmin) * (WORLD_BOUND_SCALE - 1) / 2
        out.update({"am/wide_min": (bmin - shift).numpy(), "am/wide_max": (bmax + shift).numpy()})

    # MaskCache
    mc = module.MaskCache(lo, hi, density, R.ALPHA_INIT, R.THRES, MASK_KS)
    out["mc/pooled"] = mc.density.numpy()
    out["mc/ks"] = np.int64(MASK_KS)
    for name, (shape, box, _, _) in R.MASK_CASES.items():
        if max(shape) > 32:
            continue
        axes = [torch.linspace(float(np.float32(box[a])), float(np.float32(box[3 + a])), shape[a]) for a in range(3)]
        mask = mc(torch.stack(torch.meshgrid(*axes, indexing="ij"), -1))
        out[f"mc/{name}/mask"] = mask.numpy()
        out[f"mc/{name}/box"] = np.float32(box)

    # DenseGrid.scale_volume_grid
    for ch in (1, 6):
        case = ((5, 7, 3), (13, 9, 4), ch)
        v = R.resample_input(case)
        g = module.DenseGrid(ch, torch.tensor(case[0]), lo, hi)
        with torch.no_grad():
            g.grid.copy_(torch.from_numpy(v).permute(3, 0, 1, 2)[None])
        g.scale_volume_grid(torch.tensor(case[1]))
        out[f"up/c{ch}/in"] = v
        out[f"up/c{ch}/out"] = g.grid.detach().numpy()

    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} B): {out['am/active']} active nodes, box {bmin.tolist()} .. {bmax.tolist()}, "
          f"masks {[int(v.sum()) for k, v in out.items() if k.endswith('/mask')]}")


if __name__ == "__main__":
    main()
