"""Float64 restatement of the camera-ray formulas (esr_nerf_amd/csrc/camera_ray.h, csrc/camera.hip) and the binary32 colour
recipe, for the camera tests (numpy only; no kernels, no GPU).

    pixel p of a W x H image: i = p % W, j = p // W;  px = ((i + 0.5) - cx) / fx, py = ((j + 0.5) - cy) / fy, pz = 1
    d = R (px, py, pz),  o = t,  viewdir = d / max(|d|, 1e-12)               R | t = the view's 3x4 camera-to-world matrix

The inputs (poses, fx, fy, cx, cy) are binary32 values and enter the float64 chain exactly, so the difference to a binary32
evaluation is rounding alone.  Bounds, with U = 2^-24 (half an ulp of 1):

    |rays_d   - d64|  <= K_D * U * sum_k |R_k pix_k|      per component
    |viewdirs - v64|  <= K_V * U                          per component

K_D and K_V come from the REFERENCE's own binary32 error, not from the kernels: the worst such ratio of (a) the
reference-generated record tests/golden/camera_rays.npz (the loader's float32 ``rays_d`` / ``viewdirs`` against this file's
float64) and (b) the loader's expressions -- ``torch.sum(pixel[:, None, :] * pose[..., None, :3, :3], -1)`` and
``F.normalize`` -- on 4096 seeded random poses (``measure()`` below, CPU), doubled because a different summation order or a
contraction is as legitimate as the reference's, and rounded up to an integer.  Measured by ``python tests/camera_ref.py``:

    rays_d    golden 1.38   random poses 3.11   -> K_D = ceil(2 * 3.11) = 7
    viewdirs  golden 1.60   random poses 2.28   -> K_V = ceil(2 * 2.28) = 5

(first-order expectation: a term R_k pix_k carries the difference's, the quotient's and the product's rounding, the two sums
add two more: at most 5 U relative to sum_k |R_k pix_k|, 3.1 seen; a unit vector's component inherits d's error through the
quotient, the norm's at half weight, and one rounding of its own).
"""
import math

import numpy as np

U = 2.0 ** -24
K_D = 7
K_V = 5
MEASURED = {"rays_d": {"golden": 1.38, "random": 3.11}, "viewdirs": {"golden": 1.60, "random": 2.28}}

BLENDER2OPENCV = np.diag([1.0, -1.0, -1.0, 1.0])


def blender_intrinsics(camera_angle_x, width, height):
    """(fx, fy, cx, cy) as binary32 values held in float64: data/esrnerf/esrnerf.py:39-41,54-55 -- the focal length is a
    float64 Python number and the loader's tensor-by-scalar arithmetic rounds it (and W / 2, H / 2) to the tensor's float32"""
    flen = width / 2.0 / math.tan(float(camera_angle_x) / 2.0)
    return tuple(float(np.float32(v)) for v in (flen, flen, width * 0.5, height * 0.5))


def blender_poses(transform_matrices):
    """float32 [V, 3, 4] camera-to-world of the kernels' convention: float32(matrix) @ blender2opencv (esrnerf.py:151,253;
    the product only flips the signs of two columns, so it is exact)"""
    m = np.asarray(transform_matrices, np.float64).astype(np.float32).astype(np.float64)
    return (m @ BLENDER2OPENCV)[:, :3, :4].astype(np.float32)


def rays64(poses, fx, fy, cx, cy, width, height):
    """poses float32 [V, 3, 4] -> dict(o, d, v: float64 [V*H*W, 3]; dabs: sum_k |R_k pix_k| [V*H*W, 3])"""
    P = np.asarray(poses, np.float64)
    p = np.arange(width * height)
    i, j = p % width, p // width
    pix = np.stack([((i + 0.5) - cx) / fx, ((j + 0.5) - cy) / fy, np.ones(len(p))], -1)          # [HW, 3]
    terms = P[:, None, :, :3] * pix[None, :, None, :]                                            # [V, HW, 3(a), 3(k)]
    d = terms.sum(-1).reshape(-1, 3)
    dabs = np.abs(terms).sum(-1).reshape(-1, 3)
    o = np.broadcast_to(P[:, None, :, 3], (len(P), len(p), 3)).reshape(-1, 3)
    nrm = np.maximum(np.sqrt((d * d).sum(-1, keepdims=True)), 1e-12)
    return dict(o=o, d=d, v=d / nrm, dabs=dabs)


def ratios(rays_d, viewdirs, ref):
    """worst |rays_d - d64| / (U dabs) and |viewdirs - v64| / U"""
    diff = np.abs(np.asarray(rays_d, np.float64) - ref["d"])
    with np.errstate(divide="ignore", invalid="ignore"):          # a component whose three terms are all 0 must be exact
        rd = np.where(diff == 0, 0.0, diff / (U * ref["dabs"]))
    rv = np.abs(np.asarray(viewdirs, np.float64) - ref["v"]) / U
    return float(rd.max()), float(rv.max())


def check_rays(rays_o, rays_d, viewdirs, ref):
    """-> (worst d ratio, worst viewdir ratio); asserts the origins exact and both bounds"""
    assert np.array_equal(np.asarray(rays_o), ref["o"].astype(np.float32)), "rays_o differ from the poses' translations"
    rd, rv = ratios(rays_d, viewdirs, ref)
    assert rd <= K_D, f"rays_d: worst |d - d64| / (U sum|R pix|) = {rd:.3f} > K_D = {K_D}"
    assert rv <= K_V, f"viewdirs: worst |v - v64| / U = {rv:.3f} > K_V = {K_V}"
    return rd, rv


# ---- colours ---------------------------------------------------------------------------------------------------------------
def uint8_table():
    return (np.arange(256) / 255.0).astype(np.float32)


def composite32(c, a, white_bg):
    """The binary32 recipe of the batch kernel on uint8 arrays c (colour) and a (alpha): table lookups, then
    c * a + (1 - a) * white_bg as four separately rounded float32 operations (numpy float32 arithmetic does not fuse)"""
    t = uint8_table()
    cf, af = t[np.asarray(c)], t[np.asarray(a)]
    wb = np.float32(white_bg)
    prod = (cf * af).astype(np.float32)
    inv = (np.float32(1.0) - af).astype(np.float32)
    return (prod + (inv * wb).astype(np.float32)).astype(np.float32)


def composite_rgba(rgba, white_bg):
    """rgba uint8 [n, 4] -> float32 [n, 3]"""
    rgba = np.asarray(rgba)
    return composite32(rgba[:, :3], rgba[:, 3:4], white_bg)


# ---- seeded cameras the GPU tests and the host test share -----------------------------------------------------------------
def look_at_cv(eye, target, up=(0.0, 0.0, 1.0)):
    """float32 [3, 4] camera-to-world, x right, y down, z forward (the kernels' convention)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    m = np.zeros((3, 4))
    m[:, 0], m[:, 1], m[:, 2], m[:, 3] = x, np.cross(z, x), z, eye
    return m.astype(np.float32)


def intrinsics_set():
    """The second camera set of the tests: 2 views of 5 x 3 through ``from_intrinsics``, fx != fy, off-centre principal point"""
    poses = np.stack([look_at_cv((1.7, -2.2, 1.1), (0.0, 0.1, 0.0)), look_at_cv((-2.4, 0.6, 0.8), (0.2, 0.0, -0.1))])
    K = np.array([[6.3, 0.0, 2.1], [0.0, 5.1, 1.9], [0.0, 0.0, 1.0]])
    return poses, K, 5, 3


FILTER_EYES = [(2.3, -1.2, 1.4), (-1.9, 2.0, 0.9), (0.4, 2.6, -1.1)]      # around the slab of tests/ray_filter_ref.py


def filter_set():
    """Cameras for the filter test on ray_filter_ref's slab (box (-1,-1,-.25)..(1,1,.25)): 3 views of 24 x 20, wide enough
    that some rays miss the box and some cross its occupied part -- the kept share lies strictly between 0 and 1 (checked
    on the CPU in tests/test_camera_host.py)"""
    poses = np.stack([look_at_cv(e, (0.1, -0.05, 0.0)) for e in FILTER_EYES])
    K = np.array([[17.0, 0.0, 12.0], [0.0, 17.0, 10.0], [0.0, 0.0, 1.0]])
    return poses, K, 24, 20


# ---- where K_D and K_V come from ------------------------------------------------------------------------------------------
def measure(golden_path, n_poses=4096, seed=0):
    import torch
    import torch.nn.functional as F
    with np.load(golden_path) as z:
        g = {k: z[k] for k in z.files}
    W, H = int(g["width"]), int(g["height"])
    ref = rays64(blender_poses(g["transform_matrices"]), *blender_intrinsics(g["camera_angle_x"], W, H), W, H)
    out = {"golden": ratios(g["rays_d"], g["viewdirs"], ref)}
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n_poses, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, zq = q.T
    R = np.stack([1 - 2 * (y * y + zq * zq), 2 * (x * y - zq * w), 2 * (x * zq + y * w),
                  2 * (x * y + zq * w), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - x * w),
                  2 * (x * zq - y * w), 2 * (y * zq + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    poses = np.concatenate([R, rng.uniform(-4, 4, (n_poses, 3, 1))], -1).astype(np.float32)
    W, H = 9, 7
    fx, fy, cx, cy = (float(np.float32(v)) for v in (7.7, 6.9, 4.3, 3.6))
    i, j = torch.meshgrid(torch.arange(W), torch.arange(H), indexing="xy")
    i, j = i + 0.5, j + 0.5
    pixel = torch.stack([(i - cx) / fx, (j - cy) / fy, torch.ones_like(i)], -1).view(W * H, 3)          # dtu.py:75-86
    pose = torch.from_numpy(poses)
    rays_d = torch.sum(pixel[:, None, :] * pose[..., None, :3, :3], dim=-1)                              # dtu.py:210
    viewdirs = F.normalize(rays_d, dim=-1)
    out["random"] = ratios(rays_d.reshape(-1, 3).numpy(), viewdirs.reshape(-1, 3).numpy(), rays64(poses, fx, fy, cx, cy, W, H))
    return out


if __name__ == "__main__":
    import os
    m = measure(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera_rays.npz"))
    for k, (rd, rv) in m.items():
        print(f"{k:8s} rays_d {rd:.3f}  viewdirs {rv:.3f}")
    print("K_D =", math.ceil(2 * max(v[0] for v in m.values())), " K_V =", math.ceil(2 * max(v[1] for v in m.values())))
