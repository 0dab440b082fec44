"""Write tests/golden/edit_rays.npz: the reference's own ``PDRA.filter_edit_rays`` (app/fine/pdra.py:934-1045) and
``RayGroupManager`` (utils2/utils.py:122-303) on small seeded cases.

    python tools/gen_edit_rays_golden.py            (CPU host with the reference tree and scipy)

``app/fine/pdra.py`` and ``utils2/utils.py`` are loaded by path with their third-party imports (cv2, imageio, trimesh,
wandb, hydra, omegaconf, ...) stubbed.  The method is called unbound on a stand-in ``self``: ``train_dataset.image_size``,
``focal_length``, ``device``, ``mask_dilation_ks``, ``eval_bs`` and a renderer whose ``eval_esp`` hands the case's recorded
points back chunk by chunk (``eval_esp`` itself is pinned against the reference in tests/test_gpu_lts_path.py).

OpenCV is not installed where this runs.  ``cv2.dilate`` is supplied from ``scipy.ndimage.maximum_filter`` with OpenCV's
documented definition for ``np.ones((ks, ks))``, ``iterations=1``: anchor ks // 2, i.e. the window -(ks // 2) .. ks - 1 -
ks // 2, outside pixels taking no part; the tool asserts that it equals the independent restatement of
tests/relight_ref.py.  The dilation is therefore pinned by the definition and two restatements, not by an OpenCV run.

Only data goes into the file: per case the inputs, the dilated masks, the float32 (u, v) the reference computed, the keep
flags and the three label arrays (in the uncertain group's order), and the sampler's index vectors and per-key group
arrays afterwards.  The tests only read the .npz.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF_ROOT = os.environ.get("ESR_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "edit_rays.npz")
DATA_KEYS = ["rgbs", "rays_o", "rays_d", "viewdirs", "em_modes"]


def _cv2_dilate(src, kernel, iterations=1):
    from scipy import ndimage
    assert iterations == 1 and kernel.ndim == 2 and kernel.shape[0] == kernel.shape[1] and (kernel == 1).all()
    ks = kernel.shape[0]
    src = np.asarray(src)
    size = (ks, ks) + (1,) * (src.ndim - 2)
    # scipy centres an even window at size // 2 as well (origin 0): offsets -(ks // 2) .. ks - 1 - ks // 2
    out = ndimage.maximum_filter(src, size=size, mode="constant", cval=-np.inf)
    return out[..., 0] if src.ndim == 3 and src.shape[2] == 1 else out       # cv2 drops a single channel


def load_reference():
    """(pdra module, utils module) of the reference, loaded by path"""
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        m.__path__ = []
        sys.modules[name] = m
        return m

    anything = type("Anything", (), {})
    stub("cv2", dilate=_cv2_dilate)
    for name in ("imageio", "trimesh", "hydra", "hydra.core"):
        stub(name)
    stub("wandb", config={"system": {"debug": True, "tqdm_iters": 10}})
    stub("hydra.core.hydra_config", HydraConfig=anything)
    stub("omegaconf", DictConfig=anything, OmegaConf=anything)
    stub("app", AppClass=object)
    stub("app.fine")
    stub("app.fine.model", ESRNeRF=anything)
    stub("app.utils")
    stub("app.utils.optimizer", CosineLR=anything, create_optimizer_or_freeze_model=None)
    stub("data", DataClass=anything)
    stub("utils2")
    stub("utils2.image", apply_gamma_curve=None)
    stub("utils2.manager", save_cfg=None)
    stub("utils2.metric", IoU=None, loss2psnr=None, rgb_lpips=None, rgb_ssim=None)

    def by_path(modname, rel):
        spec = importlib.util.spec_from_file_location(modname, os.path.join(REF_ROOT, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[modname] = mod
        spec.loader.exec_module(mod)
        return mod

    utils = by_path("utils2.utils", "utils2/utils.py")
    return by_path("_ref_pdra", "app/fine/pdra.py"), utils


class _CaptureUV(torch.overrides.TorchFunctionMode):
    """Records the operand of ``img_coord < 0`` (pdra.py:997): the float32 (u, v) of every chunk"""

    def __init__(self):
        super().__init__()
        self.uv = []

    def __torch_function__(self, func, types_, args=(), kwargs=None):
        if getattr(func, "__name__", "") in ("lt", "__lt__") and len(args) == 2 and isinstance(args[0], torch.Tensor) \
                and args[0].dim() == 2 and args[0].shape[1] == 2 and not isinstance(args[1], torch.Tensor) and args[1] == 0:
            self.uv.append(args[0].detach().clone())
        return func(*args, **(kwargs or {}))


class _Renderer:
    def __init__(self, esp, bs):
        self.chunks = list(torch.from_numpy(esp).split(bs))

    def eval(self):
        return self

    def eval_esp(self, rays_o, rays_d, viewdirs):
        out = self.chunks.pop(0)
        assert len(out) == len(rays_o)
        return out.clone()


def soft_masks(rng, h, w, shapes):
    """Float masks with fractional edges: boxes / discs blurred by a 3 x 3 mean, exact zeros away from them"""
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for kind, cy, cx, r in shapes:
        m = ((np.abs(yy - cy) <= r) & (np.abs(xx - cx) <= r)) if kind == "box" else ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r)
        m = m.astype(np.float64)
        pad = np.pad(m, 1)
        blur = sum(pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
        out.append((blur * (0.5 + 0.5 * rng.random())).astype(np.float32))
    return np.stack(out)


def look_at_pose(eye, target):
    """Camera-to-world [4, 4] of a camera at ``eye`` whose -z axis points at ``target`` (the datasets' convention)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, y, z, eye
    return P.astype(np.float32)


def frustum_points(rng, pose, f, w, h, n, spread):
    """World points whose projection is spread over ``spread`` x the image around its centre, at depths 1 .. 4 in front"""
    K = np.array([[-f, 0, w / 2 - 0.5], [0, f, h / 2 - 0.5], [0, 0, 1.0]])
    u = (w / 2 - 0.5) + (rng.random(n) - 0.5) * w * spread
    v = (h / 2 - 0.5) + (rng.random(n) - 0.5) * h * spread
    d = 1.0 + 3.0 * rng.random(n)
    # K cam = (u, v, 1) * cam_z; the sign of cam_z cancels in the projection, the datasets' cameras look along -z
    cam = np.linalg.solve(K, np.stack([u, v, np.ones(n)])) * -d
    world = pose[:3, :3].astype(np.float64) @ cam + pose[:3, 3:4]
    return world.T.astype(np.float32)


def integer_points(pose, f, w, h, rng, n):
    """Points that project EXACTLY onto integer (and a few half-integer) pixel coordinates in float32 under any rounding
    order: axis-aligned camera with small-integer translation, focal length and depths powers of two"""
    t = pose[:3, 3].astype(np.float64)
    u = rng.integers(-3, max(h, w) + 3, n).astype(np.float64)
    v = rng.integers(-3, max(h, w) + 3, n).astype(np.float64)
    half = rng.random(n) < 0.15
    u[half] += 0.5
    v[rng.random(n) < 0.15] += 0.5
    d = -np.exp2(rng.integers(0, 3, n)).astype(np.float64)                      # cam z = -1, -2, -4
    cam = np.stack([-(u - (w / 2 - 0.5)) * d / f, (v - (h / 2 - 0.5)) * d / f, d], 1)
    pts = (cam + t).astype(np.float32)
    assert (pts.astype(np.float64) == cam + t).all()
    return pts


def build_cases():
    rng = np.random.default_rng(20)
    out = {}
    # name: image (w, h), conditions in an order where the field-wise override matters, every mode present over the cases
    spec = {
        "wide": dict(size=(52, 40), modes=[2, 3, 0], shapes=[("disc", 18, 20, 7), ("box", 20, 27, 6), ("box", 5, 2, 4)]),
        "tall": dict(size=(40, 52), modes=[4, 1, 2, 3, 0],
                     shapes=[("disc", 20, 18, 8), ("box", 30, 20, 5), ("disc", 24, 24, 6), ("box", 26, 14, 7), ("box", 49, 36, 4)]),
        "integer": dict(size=(52, 40), modes=[2, 3, 4, 0], shapes=[("box", 12, 14, 6), ("disc", 16, 20, 7), ("box", 30, 30, 5),
                                                                     ("box", 2, 37, 3)]),
    }
    for name, s in spec.items():
        w, h = s["size"]
        n_cond = len(s["modes"])
        n_all, n_unc, bs = 3000, 2200, 512
        if name == "integer":
            f = 64.0
            pose = np.eye(4, dtype=np.float32)
            pose[:3, 3] = [2.0, -1.0, 3.0]
            esp = integer_points(pose, f, w, h, rng, n_unc)
        else:
            f = 55.0 if name == "wide" else 47.5
            pose = look_at_pose([2.2, -1.4, 1.7] if name == "wide" else [-1.9, 2.4, 1.1], [0.1, 0.0, 0.2])
            esp = np.concatenate([frustum_points(rng, pose, f, w, h, n_unc - 300, 1.6),     # inside and outside the frustum
                                  frustum_points(rng, pose, f, w, h, 200, 0.5),
                                  np.zeros((100, 3), np.float32)])                          # rays without a surviving sample
            esp = esp[rng.permutation(n_unc)]
        perm = rng.permutation(n_all)
        data = dict(rgbs=(np.arange(n_all * 3).reshape(n_all, 3) % 251 / 250).astype(np.float32),
                    rays_o=(np.arange(n_all * 3).reshape(n_all, 3) % 17 / 16).astype(np.float32),
                    rays_d=(np.arange(n_all * 3).reshape(n_all, 3) % 13 / 8 - 0.75).astype(np.float32),
                    viewdirs=(np.arange(n_all * 3).reshape(n_all, 3) % 11 / 8 - 0.5).astype(np.float32),
                    em_modes=(np.arange(n_all) % 2).astype(np.int64))
        out[name] = dict(image_size=np.array([w, h], np.int64), focal=np.float64(f), ks=np.int64(10), eval_bs=np.int64(bs),
                         pose=pose, esp=esp, em_masks=soft_masks(rng, h, w, s["shapes"]),
                         em_modes_cond=np.array(s["modes"], np.int64),
                         em_intensities_cond=(0.25 + 2.0 * rng.random(n_cond)).astype(np.float32),
                         em_colors_cond=rng.random((n_cond, 3)).astype(np.float32),
                         uncert_idxs_in=perm[:n_unc].astype(np.int64), cert_idxs_in=perm[n_unc:].astype(np.int64),
                         **{f"data/{k}": v for k, v in data.items()})
    return out


def run_case(pdra, utils, c):
    import relight_ref
    w, h = (int(x) for x in c["image_size"])
    cfg = types.SimpleNamespace(system=types.SimpleNamespace(device="cpu", data_preload="gpu"))
    data = {k: torch.from_numpy(c[f"data/{k}"].copy()) for k in DATA_KEYS}
    sampler = utils.RayGroupManager(cfg, data, list(DATA_KEYS), 64, 64, uncert_data_idxs=torch.from_numpy(c["uncert_idxs_in"]),
                                    cert_data_idxs=torch.from_numpy(c["cert_idxs_in"]))
    me = types.SimpleNamespace(train_dataset=types.SimpleNamespace(image_size=(w, h), focal_length=float(c["focal"])),
                               device="cpu", mask_dilation_ks=int(c["ks"]), eval_bs=int(c["eval_bs"]),
                               renderer=_Renderer(c["esp"], int(c["eval_bs"])))
    test_data = dict(poses=torch.from_numpy(c["pose"]), em_masks=torch.from_numpy(c["em_masks"]).reshape(-1),
                     em_modes=torch.from_numpy(c["em_modes_cond"]), em_intensities=torch.from_numpy(c["em_intensities_cond"]),
                     em_colors=torch.from_numpy(c["em_colors_cond"]))
    seen = {}
    real_filter = sampler.filter

    def recording_filter(mask):
        seen.update(keep=mask.clone(), **{k: sampler.uncert_data[k].clone() for k in ("em_modes", "em_colors", "em_intensities")})
        return real_filter(mask)

    sampler.filter = recording_filter
    real_dilate = sys.modules["cv2"].dilate
    dilated = {}

    def recording_dilate(src, kernel, iterations=1):
        dilated["out"] = real_dilate(src, kernel, iterations=iterations)
        return dilated["out"]

    sys.modules["cv2"].dilate = pdra.cv2.dilate = recording_dilate
    try:
        with _CaptureUV() as cap:
            pdra.PDRA.filter_edit_rays(me, sampler, test_data)
    finally:
        sys.modules["cv2"].dilate = pdra.cv2.dilate = real_dilate
    dil = np.ascontiguousarray(np.moveaxis(dilated["out"].reshape(h, w, -1), 2, 0))
    assert np.array_equal(dil, relight_ref.dilate(c["em_masks"], int(c["ks"]))), "the two dilation restatements differ"
    rec = dict(c, w2c=torch.inverse(torch.from_numpy(c["pose"])).numpy(), dilated=dil, ref_uv=torch.cat(cap.uv).numpy(),
               keep=seen["keep"].numpy(), em_modes=seen["em_modes"].numpy(), em_colors=seen["em_colors"].numpy(),
               em_intensities=seen["em_intensities"].numpy(), uncert_data_idxs=sampler.uncert_data_idxs.numpy(),
               cert_data_idxs=sampler.cert_data_idxs.numpy(), keys=np.array(json.dumps(sampler.keys)))
    for k in sampler.keys:
        rec[f"uncert/{k}"], rec[f"cert/{k}"] = sampler.uncert_data[k].numpy(), sampler.cert_data[k].numpy()
    assert len(rec["ref_uv"]) == len(c["esp"])
    return rec


def main():
    import relight_ref
    pdra, utils = load_reference()
    out, names = {}, []
    for name, c in build_cases().items():
        rec = run_case(pdra, utils, c)
        names.append(name)
        out.update({f"{name}/{k}": v for k, v in rec.items()})
    out["cases"] = np.array(json.dumps(names))
    np.savez_compressed(OUT, **out)
    z = np.load(OUT)
    d = relight_ref.delta(z)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} B), delta = {d:.3e} px")
    for name in names:
        c = relight_ref.case(z, name)
        for dtype in (np.float64, np.float32):
            r = relight_ref.case_label(c, dtype)
            clear = r["clearance"] > d
            bad = sum(int((np.asarray(r[k]) != c[k]).reshape(len(clear), -1).any(1)[clear].sum())
                      for k in ("keep", "em_modes", "em_colors", "em_intensities"))
            allbad = sum(int((np.asarray(r[k]) != c[k]).reshape(len(clear), -1).any(1).sum())
                         for k in ("keep", "em_modes", "em_colors", "em_intensities"))
            print(f"  {name} {np.dtype(dtype).name}: kept {int(c['keep'].sum())} of {len(clear)}, modes "
                  f"{np.bincount(c['em_modes'], minlength=5).tolist()}, unclear {100 * (1 - clear.mean()):.2f} %, mismatches on clear rays "
                  f"{bad}, on all rays {allbad}")


if __name__ == "__main__":
    main()
