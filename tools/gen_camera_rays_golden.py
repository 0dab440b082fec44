"""Write tests/golden/camera_rays.npz: what the reference's own ESR-NeRF loader (data/esrnerf/esrnerf.py, phase "train")
makes of a tiny dataset -- ``rays_o``, ``rays_d``, ``viewdirs``, ``rgbs`` (for both ``white_bg`` settings) and ``em_modes`` --
beside the inputs it was given: the transform matrices, ``camera_angle_x`` and the raw RGBA bytes.

    python tools/gen_camera_rays_golden.py            (CPU host with the reference tree)

The tool writes a temporary ESR-NeRF-style dataset (``transforms/transforms_train.json`` plus RGBA PNGs through PIL): 3 views
of 13 x 7 pixels, the first pose axis-aligned, the other two oblique; alpha takes 0, 255 and values in between; the views'
light modes are off / on / off.  It then constructs ``data.esrnerf.ESRNeRF(cfg, "train")`` from the reference tree, once per
``white_bg``.  Modules the loader imports but the train phase never calls are stubbed the way oracle/ref_import.py stubs
modules: ``cv2`` (read only by the test phases' EXR code), ``omegaconf`` and ``wandb`` (``wandb.config`` tells ``tqdm_safe`` to
hand the plain iterator back).

The DTU loader (data/dtu/dtu.py) cannot be run this way: its ``load_K_Rt_from_P`` needs ``cv2.decomposeProjectionMatrix``.  Its
intrinsics form (``Cameras.from_intrinsics``: fx != fy, an off-centre principal point) is therefore covered by the float64
restatement of tests/camera_ref.py only, not by a reference-generated record.

Only data goes into the file; the tests only read the .npz.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "camera_rays.npz")
REF_ROOT = os.environ.get("ESR_REFERENCE_ROOT", "/root/reference")
WIDTH, HEIGHT = 13, 7
MODES = ["off", "on", "off"]


def blender_look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """4x4 camera-to-world in Blender's convention (x right, y up, camera looks along -z)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, eye
    return m


def dataset():
    rng = np.random.default_rng(17)
    axis = np.eye(4)
    axis[:3, 3] = (0.25, -0.5, 4.0)                                  # axis-aligned: looks straight down -z
    poses = [axis, blender_look_at((2.9, -2.1, 1.7), (0.1, 0.05, -0.1)), blender_look_at((-1.3, 3.4, 0.9), (0.0, -0.2, 0.15))]
    images = rng.integers(0, 256, (len(poses), HEIGHT, WIDTH, 4), dtype=np.uint8)
    alpha = images[..., 3]
    pick = rng.random(alpha.shape)
    alpha[pick < 0.25] = 0
    alpha[pick > 0.75] = 255
    images[0, 0, 0] = (0, 255, 1, 254)                               # the extremes beside each other
    images[2, -1, -1] = (255, 0, 254, 1)
    return np.stack(poses), 0.6911112070083618, images


def stub_modules():
    om = types.ModuleType("omegaconf")
    om.DictConfig = type("DictConfig", (dict,), {})
    om.OmegaConf = type("OmegaConf", (), {})
    sys.modules.setdefault("omegaconf", om)
    wb = types.ModuleType("wandb")
    wb.config = {"system": {"debug": True, "tqdm_iters": 10}}
    sys.modules.setdefault("wandb", wb)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))           # absent here; unused in the train phase


def main():
    from PIL import Image
    if not os.path.isdir(os.path.join(REF_ROOT, "data", "esrnerf")):
        sys.exit(f"reference not found at {REF_ROOT}")
    stub_modules()
    sys.path.insert(0, REF_ROOT)
    from data.esrnerf.esrnerf import ESRNeRF
    poses, angle, images = dataset()
    out = dict(transform_matrices=poses, camera_angle_x=np.float64(angle), rgba=images.reshape(-1, 4),
               width=np.int64(WIDTH), height=np.int64(HEIGHT))
    with tempfile.TemporaryDirectory() as root:
        scene = os.path.join(root, "tiny")
        os.makedirs(os.path.join(scene, "transforms"))
        os.makedirs(os.path.join(scene, "train"))
        frames = []
        for v, (pose, img) in enumerate(zip(poses, images)):
            Image.fromarray(img, "RGBA").save(os.path.join(scene, "train", f"r_{v}.png"))
            frames.append(dict(file_path=f"train/r_{v}", transform_matrix=pose.tolist(), lights=[dict(mode=MODES[v])]))
        with open(os.path.join(scene, "transforms", "transforms_train.json"), "w") as f:
            json.dump(dict(camera_angle_x=angle, frames=frames), f)
        for white_bg in (True, False):
            attr = lambda **kw: types.SimpleNamespace(**kw)
            cfg = attr(system=attr(device="cpu"),
                       data=attr(root=root, scene="tiny", resize=None, batch_type="nerf", white_bg=white_bg))
            ds = ESRNeRF(cfg, "train")
            assert ds.image_size == (WIDTH, HEIGHT)
            c = {k: v.numpy() for k, v in ds.all_data.items()}
            tag = "white" if white_bg else "black"
            out[f"rgbs_{tag}"] = c["rgbs"]
            rays = dict(rays_o=c["rays_o"], rays_d=c["rays_d"], viewdirs=c["viewdirs"], em_modes=c["em_modes"],
                        poses_f32=c["poses"], focal=np.float64(ds.focal_length))
            for k, v in rays.items():
                assert k not in out or np.array_equal(out[k], v), k          # the rays do not depend on the background
                out[k] = v
    n = len(poses) * WIDTH * HEIGHT
    assert out["rays_d"].shape == (n, 3) and out["rays_d"].dtype == np.float32 and out["em_modes"].dtype == np.int64
    assert out["rgbs_white"].shape == (n, 3) and out["rgbs_white"].dtype == np.float32
    a = out["rgba"][:, 3]
    assert (a == 0).any() and (a == 255).any() and ((a > 0) & (a < 255)).any()
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {n} rays, {os.path.getsize(OUT)} B")


if __name__ == "__main__":
    main()
