"""tests/golden/surfenv.npz: what the reference computes for the pieces that the environment light on the surface restates
(csrc/surfenv.hip, sources.hemisphere_directions / environment_light; tests/surfenv_ref.py).  Data only, a few KB:

  table_<n>     fibonacci_spiral_samples_on_unit_hemisphere(n) for n in 1, 2, 16, 17, 128, 256 (float32 [n, 3])
  flip_normals  five normals (float32 [5, 3]) and  flip_dirs  diffuse_scattering_fib(normals, 16) (float32 [5, 16, 3])
  sg_mus / sg_lambdas / sg_lobes   a seeded SphericalGaussian(48, "softplus"),  sg_dirs  64 unit directions (float32) and
  sg_out        its output on them (float32 [64, 3])

The reference's two files (app/utils/pbr/functions.py, module.py) are imported at run time from ESR_REFERENCE_ROOT; they
need torch and numpy alone.

    [ESR_REFERENCE_ROOT=/path/to/reference] python tools/gen_surfenv_golden.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_import import REF_ROOT  # noqa: E402  (the one owner of where the reference lies: ESR_REFERENCE_ROOT)
TABLES = (1, 2, 16, 17, 128, 256)


def by_path(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF_ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    fn = by_path("_ref_pbr_functions", "app/utils/pbr/functions.py")
    md = by_path("_ref_pbr_module", "app/utils/pbr/module.py")
    out = {f"table_{n}": fn.fibonacci_spiral_samples_on_unit_hemisphere(n).numpy() for n in TABLES}
    # the first is orthogonal to no direction, the last lies in the plane z = 0 and one looks down
    normals = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.6, -0.48, 0.64], [-0.8, 0.6, 0.0], [0.28, 0.0, -0.96]])
    out["flip_normals"] = normals.numpy()
    out["flip_dirs"] = fn.diffuse_scattering_fib(normals, 16).numpy()
    torch.manual_seed(20)
    sg = md.SphericalGaussian(48, "softplus")
    d = torch.nn.functional.normalize(torch.randn(64, 3), dim=-1)
    with torch.no_grad():
        out.update(sg_mus=sg.mus.detach().numpy(), sg_lambdas=sg.lambdas.detach().numpy(), sg_lobes=sg.lobes.detach().numpy(),
                   sg_dirs=d.numpy(), sg_out=sg(d).numpy())
    for k, x in out.items():
        assert x.dtype == np.float32, (k, x.dtype)
    path = os.path.join(ROOT, "tests", "golden", "surfenv.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", {k: x.shape for k, x in out.items()})


if __name__ == "__main__":
    sys.exit(main())
