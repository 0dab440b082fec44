"""Write tests/golden/ray_filter.npz: the reference's own ``VoxurfC.sample_ray_ori``,
``VoxurfC.filter_training_rays_in_maskcache_sampling`` (app/coarse/model/voxurfc.py:426-481) and
``VoxurfF.filter_training_rays_in_maskcache_sampling`` in both ``sdf_random_init`` branches
(app/fine/model/voxurff.py:463-537) on CPU, on the seeded prune-mask slab of tests/ray_filter_ref.py.

    python tools/gen_ray_filter_golden.py            (CPU host with the reference tree)

The reference classes are loaded the way oracle/gen_golden.py loads them (oracle/ref_import.py).  Rays: pinhole-camera rays
from four poses around the box plus hand-placed families -- a direction component exactly 0, rays that miss the box, origins
inside the box, rays whose t-range the model's ``far`` cuts (fixed sampler only), rays that graze along the mask's empty slab
so that the first kept step lies beyond 64 and beyond 128 steps, and rays whose only kept steps are their last few in-box
samples (within their last 8 in-box ones).  Candidates that the float64 classifier (tests/ray_filter_ref.py) calls marginal under any of the three
configurations are left out BEFORE the reference runs (a choice of inputs); the tool then asserts that no ray of the file is
marginal, that the reference's flags equal the classifier's on every ray, and that every family is present.  That is why the
tests may demand bit-equal flags on this file.

Only data goes into the file: the rays, ``far``, the three flag vectors, and ``pts / mask / step`` of ``sample_ray_ori`` for
a handful of rays.  The tests only read the .npz.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "ray_filter.npz")
TAIL = 8          # "the last few samples": the first kept step is among the last TAIL in-box steps


def candidates():
    import ray_filter_ref as R
    rng = np.random.default_rng(11)
    fam = {}
    ros, rds = [], []
    for eye in R.POSES:
        ro, rd = R.camera_rays(R.look_at(eye, (0.1, -0.05, 0.0)), 10, 12, 9.0, rng.random((2, 10, 12)).astype(np.float32))
        ros.append(ro)
        rds.append(rd)
    fam["camera"] = (np.concatenate(ros), np.concatenate(rds))
    n = 60
    # a direction component exactly 0 (origin inside and outside the box's extent on that axis)
    ro = np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-1.2, 1.2, n), np.full(n, 1.5)], -1)
    rd = np.stack([rng.uniform(-0.3, 0.3, n), np.zeros(n), -rng.uniform(0.5, 1.5, n)], -1)
    rd[::3, 0] = 0.0
    fam["zero"] = (ro, rd)
    # rays that miss the box
    ro = np.stack([rng.uniform(1.3, 2.0, n), rng.uniform(-2, 2, n), rng.uniform(0.5, 2.0, n)], -1)
    rd = np.stack([rng.uniform(0.1, 1.0, n), rng.uniform(-1, 1, n), rng.uniform(-0.2, 1.0, n)], -1)
    fam["miss"] = (ro, rd)
    # origins inside the box
    ro = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(-0.9, 0.9, n), rng.uniform(-0.2, 0.2, n)], -1)
    rd = rng.normal(size=(n, 3)) * rng.uniform(0.3, 2.0, (n, 1))
    fam["inside"] = (ro, rd)
    # far cuts the t-range: unit-speed rays from ~4 away whose box entry lies beyond, or whose chord straddles, far = 3.2
    ang = rng.uniform(0, 2 * np.pi, 2 * n)
    ro = np.stack([4.2 * np.cos(ang), 4.2 * np.sin(ang), rng.uniform(0.3, 0.9, 2 * n)], -1)
    tgt = np.stack([rng.uniform(-0.8, 0.8, 2 * n), rng.uniform(-0.8, 0.8, 2 * n), rng.uniform(-0.2, 0.2, 2 * n)], -1)
    rd = tgt - ro
    rd /= np.linalg.norm(rd, axis=-1, keepdims=True)
    fam["far"] = (ro, rd)
    # grazing rays along x / y inside the mask's empty z slab: late first hits, or none but the last few samples
    m = 6000
    along = rng.integers(0, 4, m)                      # 0: along x, 1: along y, 2 / 3: along the two diagonals (181 steps)
    side = rng.uniform(-0.85, 0.85, m)
    z0 = rng.uniform(0.03, 0.11, m)
    slope = rng.uniform(-0.05, 0.05, (m, 2))
    diag = along >= 2
    sgn = np.where(along == 3, -1.0, 1.0)
    ro = np.stack([np.where(along == 1, side, -1.4), np.where(along == 0, side, np.where(diag, -1.4 * sgn + 0.3 * side, -1.4)), z0], -1)
    rd = np.stack([np.where(along == 1, slope[:, 0], 1.0), np.where(along == 0, slope[:, 0], np.where(diag, sgn * (1.0 + slope[:, 0]), 1.0)),
                   slope[:, 1] * np.where(diag, 0.6, 1.0)], -1)
    rd *= rng.uniform(0.4, 1.6, (m, 1))
    fam["graze"] = (ro, rd)
    # from inside the empty slab up through the occupied layer under the top face: the only kept steps are the last few
    # in-box ones (the mask box ends ~2 steps inside the scene box, so the very last in-box samples of any ray read padding)
    ro = np.stack([rng.uniform(-0.8, 0.8, 4 * n), rng.uniform(-0.8, 0.8, 4 * n), rng.uniform(0.04, 0.09, 4 * n)], -1)
    rd = np.stack([rng.uniform(-0.3, 0.3, 4 * n), rng.uniform(-0.3, 0.3, 4 * n), rng.uniform(0.6, 1.4, 4 * n)], -1)
    fam["tail"] = (ro, rd)
    return {k: (a.astype(np.float32), b.astype(np.float32)) for k, (a, b) in fam.items()}


def main():
    import ray_filter_ref as R
    from oracle import ref_import
    ns = ref_import.load()
    coarse, fine = R.renderers("cpu", ns.VoxurfC, ns.VoxurfF)
    configs = {"coarse_fixed": (coarse, True), "fine_fixed": (fine, True), "fine_march": (fine, False)}
    scenes = {k: R.scene_of(m) for k, (m, _) in configs.items()}
    ros, rds, names = [], [], []
    for name, (ro, rd) in candidates().items():
        res = {k: R.classify(scenes[k], ro, rd, fx) for k, (_, fx) in configs.items()}
        firm = np.all([r["cls"] != R.MARGINAL for r in res.values()], 0)
        sel = firm.copy()
        if name == "graze":          # keep the interesting ones: late deciding trips and last-samples-only rays
            late = np.zeros(len(ro), bool)
            for r in res.values():
                mid = (r["first64"] >= 64) & (r["first64"] < 128)
                late |= mid & (np.cumsum(mid) <= 60)
                late |= r["first64"] >= 128
                late |= (r["first64"] >= 0) & (r["last_in64"] - r["first64"] < TAIL)
            dropped = np.all([~r["keep64"] for r in res.values()], 0)
            dropped &= np.cumsum(dropped) <= 40
            sel &= late | dropped
        print(f"{name:8s} {len(ro):5d} candidates, {int((~firm).sum()):3d} marginal left out, {int(sel.sum()):4d} taken")
        ros.append(ro[sel])
        rds.append(rd[sel])
        names += [name] * int(sel.sum())
    ro, rd = np.concatenate(ros), np.concatenate(rds)
    perm = np.random.default_rng(3).permutation(len(ro))          # families interleaved: blocks hold rays of every kind
    ro, rd, names = ro[perm], rd[perm], np.array(names)[perm]
    tro, trd = torch.from_numpy(ro), torch.from_numpy(rd)
    out = dict(rays_o=ro, rays_d=rd, family=names, far=np.float32(coarse.far), scene=np.array(R.SCENE),
               world_size=np.array(coarse.sdf.grid.shape[2:]), n_samples=np.int64(scenes["coarse_fixed"]["n_samples"]))
    stats = {}
    for key, (model, fx) in configs.items():
        if model is fine:
            model.sdf_random_init = fx
        keep = model.filter_training_rays_in_maskcache_sampling(tro, trd, 96).numpy()
        out[f"keep/{key}"] = keep
        c = R.classify(scenes[key], ro, rd, fx)
        bad, share = R.agreement(c["cls"], keep)
        assert share == 0.0, (key, share)
        assert bad == 0, (key, bad)
        stats[key] = c
        print(f"{key}: kept {int(keep.sum())} of {len(keep)}; first kept step >= 64: {int((c['first64'] >= 64).sum())}, "
              f">= 128: {int((c['first64'] >= 128).sum())}; kept on the last {TAIL} in-box samples only: "
              f"{int(((c['first64'] >= 0) & (c['last_in64'] - c['first64'] < TAIL)).sum())}; longest walk {int(c['n64'].max())}")
        assert (c["first64"] >= 128).sum() >= 3 and ((c["first64"] >= 64) & (c["first64"] < 128)).sum() >= 3, key
        assert ((c["first64"] >= 0) & (c["last_in64"] - c["first64"] < TAIL)).sum() >= 3, key
    assert (out["keep/fine_fixed"] != out["keep/fine_march"]).sum() >= 3, "far cuts no ray"
    assert ((rd == 0).any(-1)).sum() >= 10 and (names == "miss").sum() >= 10 and (names == "inside").sum() >= 10
    pick = np.concatenate([np.nonzero(names == f)[0][:2] for f in ("camera", "zero", "miss", "inside", "far", "graze", "tail")])
    pts, mask, step = coarse.sample_ray_ori(tro[pick], trd[pick])
    out.update(ori_rays=pick.astype(np.int64), ori_pts=pts.numpy(), ori_mask=mask.numpy(), ori_step=step.numpy())
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(ro)} rays, {os.path.getsize(OUT)} B")


if __name__ == "__main__":
    main()
