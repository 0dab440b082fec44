"""Write tests/golden/dtu_cd_small.npz: the reference's own utils2.metric.DTU_CD on a small synthetic DTU case.

    python tools/gen_dtu_cd_golden.py            (CPU host with the reference tree and scikit-learn)

The reference module is loaded by path, as oracle/ref_import.py loads the model files: lpips, trimesh and wandb (and the
progress-bar helper of utils2.utils) are stubbed, the mesh is a small object with ``remove_unreferenced_vertices``, and
``np.random.default_rng`` is replaced, for the call, by a generator whose ``shuffle`` applies a fixed permutation and
records it.  The case: a marching-cubes sphere (tests/mesh_ref.py) with an extra degenerate triangle and an unreferenced
vertex; an ObsMask with holes and a BB that clips the sphere (patch = 2); an stl cloud of jittered sphere points with
far outliers, cut by the ground plane.  The GPU tests only read the .npz.
"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF_ROOT = os.environ.get("ESR_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "dtu_cd_small.npz")


def case(seed=0):
    import mesh_ref
    rng = np.random.default_rng(seed)
    R, lo, hi = 30, -8.0, 8.0
    ax = np.linspace(lo, hi, R)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    c, r = (0.22, -0.14, 0.1), 6.0
    u = (r - np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)).astype(np.float32)
    v, f = mesh_ref.marching_cubes(u, 0.0)
    v = v / (R - 1) * (hi - lo) + lo
    # an unreferenced vertex in the middle of the list, and a zero-area triangle (a repeated corner)
    k = len(v) // 2
    v = np.concatenate([v[:k], [[9.0, 9.0, 9.0]], v[k:]])
    f = np.where(f >= k, f + 1, f)
    f = np.concatenate([f, [[f[0, 0], f[0, 1], f[0, 0]]]])
    obs = rng.random((9, 14, 15)) > 0.2
    bb = np.array([[-4.7, -8.4, -9.0], [0.6, 2.2, 1.4]])
    res = np.array([[1.0]])
    d = rng.standard_normal((4000, 3))
    stl = c + d / np.linalg.norm(d, axis=1, keepdims=True) * (r + 0.05 * rng.standard_normal((4000, 1)))
    far = c + rng.uniform(-40, 40, (400, 3))
    stl = np.concatenate([stl, far])
    plane = np.array([[0.3], [-0.2], [1.0], [0.5]])
    return dict(vertices=v, triangles=f, obs_mask=obs, bb=bb, res=res, stl=stl, plane=plane, patch=2, thresh=0.2,
                max_dist=20.0)


def load_metric():
    """utils2/metric.py of the reference with its unused third-party imports stubbed"""
    for name in ("lpips", "trimesh", "trimesh.points"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["trimesh"].Trimesh = object
    sys.modules["trimesh"].points = sys.modules["trimesh.points"]
    sys.modules["trimesh.points"].PointCloud = object
    wb = types.ModuleType("wandb")
    wb.config = {"system": {"debug": True, "tqdm_iters": 10}}
    sys.modules.setdefault("wandb", wb)

    class _Bar:
        def __init__(self, it, **kw):
            self.it = it

        def set_description(self, *a):
            pass

        def update(self, *a):
            pass

        def close(self):
            pass

    u2 = types.ModuleType("utils2")
    u2.__path__ = []
    uu = types.ModuleType("utils2.utils")
    uu.tqdm_safe = _Bar
    sys.modules["utils2"], sys.modules["utils2.utils"] = u2, uu
    spec = importlib.util.spec_from_file_location("ref_metric", os.path.join(REF_ROOT, "utils2", "metric.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_metric"] = mod              # the sampling pool pickles its worker function by module name
    spec.loader.exec_module(mod)
    return mod


class _Mesh:
    def __init__(self, v, f):
        self.vertices, self.faces = v, f

    def remove_unreferenced_vertices(self):
        used = np.zeros(len(self.vertices), bool)
        used[self.faces.reshape(-1)] = True
        remap = np.cumsum(used) - 1
        self.vertices, self.faces = self.vertices[used], remap[self.faces]


def main():
    metric = load_metric()
    c = case()
    rec = {}

    class _Rng:
        def shuffle(self, x, axis=0):
            assert axis == 0
            perm = np.random.Generator(np.random.PCG64(1234)).permutation(len(x))
            rec["perm"] = perm
            x[:] = x[perm]

    real = np.random.default_rng
    metric.np.random.default_rng = lambda *a, **k: _Rng()
    try:
        d2s, s2d, overall = metric.DTU_CD(_Mesh(c["vertices"].copy(), c["triangles"].copy()), c["obs_mask"], c["bb"],
                                          c["res"], c["stl"], c["plane"], max_dist=c["max_dist"], patch=c["patch"],
                                          thresh=c["thresh"])
    finally:
        metric.np.random.default_rng = real
    out = {k: np.asarray(v) for k, v in c.items()}
    out.update(perm=rec["perm"].astype(np.int32), mean_d2s=np.float64(d2s), mean_s2d=np.float64(s2d),
               overall=np.float64(overall))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} B): {len(rec['perm'])} points, d2s {d2s!r}, s2d {s2d!r}")


if __name__ == "__main__":
    main()
