"""The DVGO pre-stage's CPU side: the restatement tests/dvgo_ref.py and the CPU-resident drop-in esr_nerf_amd.dvgo.DVGO
against the reference's own DVGO (tests/golden/dvgo_small.npz, tools/gen_dvgo_golden.py); the module's parameters,
checkpoints and grid resolution; the C structs of its ABI."""
import ctypes
import os
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dvgo_ref
from conftest import ROOT, load_npz, rel_err
from esr_nerf_amd.config import alphamask_cfg
from esr_nerf_amd.dvgo import DVGO

TRAIN_KEYS = ("etc/alphainv_cum", "etc/weights", "etc/white_bg", "srgb/raw_rgb", "srgb/rgb")
EVAL_KEYS = ("etc/depth", "etc/disp", "etc/white_bg", "srgb/off_rgb", "srgb/on_rgb", "srgb/emo_rgb", "srgb/rgb")
GRIDS = ("density", "off_color", "emo_color")
FOUR = ("etc/alphainv_cum", "etc/weights", "srgb/raw_rgb", "srgb/rgb")


@pytest.fixture(scope="module")
def z():
    return load_npz("dvgo_small.npz")


def golden_model(z, device="cpu"):
    cfg = alphamask_cfg(device, num_voxels=int(z["num_voxels"]), stepsize=float(z["stepsize"]),
                        alpha_init=float(z["alpha_init"]))
    m = DVGO(cfg, float(z["near"]), float(z["far"]), torch.tensor(z["xyz_min"], device=device),
             torch.tensor(z["xyz_max"], device=device))
    m.load_state_dict({k: torch.from_numpy(z[k]) for k in GRIDS})
    return m.to(device)


def ref_consts(z):
    return SimpleNamespace(xyz_min=torch.tensor(z["xyz_min"]), xyz_max=torch.tensor(z["xyz_max"]), near=float(z["near"]),
                           far=float(z["far"]), stepsize=float(z["stepsize"]), voxel_size=torch.tensor(z["voxel_size"]),
                           act_shift=float(z["act_shift"]), N_samples=int(z["N_samples"]))


def test_golden_covers_the_cases(z):
    c = ref_consts(z)
    ro, rd = torch.from_numpy(z["rays_o"]), torch.from_numpy(z["rays_d"])
    pts, out = dvgo_ref.sample(c, ro, rd, c.N_samples, torch.from_numpy(z["jitter"]))
    assert out.all(-1).any() and (~out).any()                    # rays that miss the box, rays that hit it
    assert (rd == 0).any()                                       # exact zero direction components
    inside = ((ro > c.xyz_min) & (ro < c.xyz_max)).all(-1)
    assert inside.sum() >= 8                                     # starting inside the box
    hit = ~out.all(-1)
    assert (out[hit, -1]).all()                                  # every hitting ray leaves the box midway
    assert set(np.unique(z["em_modes"])) == {0, 1}
    assert (z["density"] == -100).any()
    assert (z["train/etc/alphainv_cum"][:, -1] == 0).any()       # T underflows behind the clamped cluster
    assert np.isfinite(z["grad/density"]).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_restatement_matches_the_reference_golden(z, dtype):
    """In float32 the restatement is the reference's arithmetic (1e-6).  In float64 the forward agrees to 1e-5; the grid
    gradients only to the reference's own float32 error: 1 - exp(-softplus(d + shift) / 2) of a low density is a
    difference of two numbers within a few ulps of 1 (alpha ~ 1e-6 carries a ~5 % rounding error in float32)."""
    c = ref_consts(z)
    tol, gtol = (1e-6, 1e-6) if dtype == torch.float32 else (1e-5, 2e-3)
    grids = {k: torch.tensor(z[k], dtype=dtype, requires_grad=True) for k in GRIDS}
    ro, rd = torch.from_numpy(z["rays_o"]), torch.from_numpy(z["rays_d"])
    res = dvgo_ref.training(c, grids, ro, rd, torch.from_numpy(z["em_modes"]), torch.from_numpy(z["jitter"]))
    for k in TRAIN_KEYS:
        assert rel_err(res[k], torch.from_numpy(z["train/" + k])) < tol, k
    up = {k: torch.from_numpy(z["up/" + k]).to(dtype) for k in FOUR}
    gr = torch.autograd.grad(sum((res[k] * up[k]).sum() for k in FOUR), [grids[k] for k in GRIDS], retain_graph=True)
    for k, g in zip(GRIDS, gr):
        assert rel_err(g, torch.from_numpy(z["grad/" + k])) < gtol, k
    loss = dvgo_ref.alphamask_loss(res, torch.from_numpy(z["rgbs"]).to(dtype))
    assert float(loss.detach()) == pytest.approx(float(z["loss"]), rel=tol)
    for k, g in zip(GRIDS, torch.autograd.grad(loss, [grids[k] for k in GRIDS])):
        assert rel_err(g, torch.from_numpy(z["loss_grad/" + k])) < gtol, k
    with torch.no_grad():
        for mode in (0, 1):
            ev = dvgo_ref.evaluate(c, grids, ro, rd, mode)
            for k in EVAL_KEYS:
                assert rel_err(ev[k], torch.from_numpy(z[f"eval{mode}/{k}"])) < tol, (mode, k)
    count, sums = dvgo_ref.count_views(c, torch.from_numpy(z["views_o"]), torch.from_numpy(z["views_d"]),
                                       tuple(z["world_size"]))
    near_one = ((sums - 1).abs() < 1e-5).any(0)[None, None]
    assert torch.equal(count[~near_one], torch.from_numpy(z["count"])[~near_one])


def test_cpu_dropin_matches_the_reference_golden(z):
    m = golden_model(z)
    assert m.N_samples == int(z["N_samples"]) and m.world_size.tolist() == z["world_size"].tolist()
    ro, rd, em = (torch.from_numpy(z[k]) for k in ("rays_o", "rays_d", "em_modes"))
    m.train()
    torch.manual_seed(7)
    res = m(rays_o=ro, rays_d=rd, em_modes=em)                   # draws the golden's jitter
    for k in TRAIN_KEYS:
        assert rel_err(res[k], torch.from_numpy(z["train/" + k])) < 1e-6, k
    up = {k: torch.from_numpy(z["up/" + k]) for k in FOUR}
    gr = torch.autograd.grad(sum((res[k] * up[k]).sum() for k in FOUR), [getattr(m, k) for k in GRIDS])
    for k, g in zip(GRIDS, gr):
        assert rel_err(g, torch.from_numpy(z["grad/" + k])) < 1e-6, k
    m.eval()
    with torch.no_grad():
        for mode in (0, 1):
            ev = m(rays_o=ro, rays_d=rd, em_modes=mode)
            assert set(ev) == set(EVAL_KEYS)
            for k in EVAL_KEYS:
                assert rel_err(ev[k], torch.from_numpy(z[f"eval{mode}/{k}"])) < 1e-6, (mode, k)
    count = m.voxel_count_views(torch.from_numpy(z["views_o"]), torch.from_numpy(z["views_d"]), 50)
    assert torch.equal(count, torch.from_numpy(z["count"]))


def test_state_dict_keys_and_shapes_match_the_golden(z):
    m = golden_model(z)
    sd = m.state_dict()
    assert list(sd) == list(GRIDS)
    for k in GRIDS:
        assert tuple(sd[k].shape) == z[k].shape and sd[k].dtype == torch.float32
        assert isinstance(getattr(m, k), torch.nn.Parameter)
    assert [n for n, _ in m.named_parameters()] == list(GRIDS)


def test_reference_format_checkpoint_loads(z, tmp_path):
    m = golden_model(z)
    # the alphamask trainer's checkpoint layout (alphamask.py: params["renderer"]["params"] and the box / near / far)
    ck = {"renderer": {"params": {k: torch.from_numpy(z[k]).clone() for k in GRIDS}, "near": float(z["near"]),
                       "far": float(z["far"]), "xyz_min": torch.from_numpy(z["xyz_min"]),
                       "xyz_max": torch.from_numpy(z["xyz_max"])}}
    path = str(tmp_path / "last.ckpt")
    torch.save(ck, path)
    p = torch.load(path)["renderer"]
    cfg = alphamask_cfg("cpu", num_voxels=int(z["num_voxels"]), stepsize=float(z["stepsize"]),
                        alpha_init=float(z["alpha_init"]))
    m2 = DVGO(cfg, p["near"], p["far"], p["xyz_min"], p["xyz_max"])
    m2.load_state_dict(p["params"])
    for k in GRIDS:
        assert torch.equal(getattr(m2, k), getattr(m, k))
    torch.save({"renderer": {"params": m2.state_dict()}}, path)
    assert set(torch.load(path)["renderer"]["params"]) == set(GRIDS)


@pytest.mark.parametrize("num_voxels", [4000, 160 ** 3 // 4, 1024000, 2 ** 21])
@pytest.mark.parametrize("box", [((-1, -1, -1), (1, 1, 1)), ((-1.3, -0.4, -2.0), (0.9, 0.45, 2.2)),
                                 ((0.1, 0.2, 0.3), (5.1, 0.7, 1.9))])
def test_grid_resolution_and_sample_count(num_voxels, box):
    lo, hi = (torch.tensor(b, dtype=torch.float32) for b in box)
    m = DVGO(alphamask_cfg("cpu", num_voxels=num_voxels), 0.1, 5.0, lo, hi)
    ext = (hi - lo).double().numpy()
    vs = float(((hi - lo).prod() / num_voxels).pow(1 / 3))
    ws = np.floor((hi - lo).numpy() / np.float32(vs)).astype(np.int64)
    assert m.world_size.tolist() == ws.tolist()
    assert abs(np.prod(ws) / num_voxels - 1) < 0.25 and np.allclose(ext / ws, vs, rtol=0.2)
    assert m.N_samples == int(np.sqrt(((ws + 1.0) ** 2).sum()) / 0.5) + 1
    assert tuple(m.density.shape) == (1, 1, *ws) and tuple(m.emo_color.shape) == (1, 3, *ws)
    assert m.act_shift == pytest.approx(np.log(1 / (1 - 1e-6) - 1))


def test_train_switches_the_forward():
    m = DVGO(alphamask_cfg("cpu", num_voxels=2000), 0.1, 5.0, -torch.ones(3), torch.ones(3))
    m.train()
    assert m.forward.__name__ == "forward_training"
    m.eval()
    assert m.forward.__name__ == "forward_evaluate"


def test_ctypes_structs_match_the_c_layout():
    from esr_nerf_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "esr_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu",'
           'sizeof(esr_dvgo_t),offsetof(esr_dvgo_t,n_samples),offsetof(esr_dvgo_t,near_),sizeof(esr_dvgo_rays_t),'
           'offsetof(esr_dvgo_rays_t,n_rays),sizeof(esr_dvgo_out_t),sizeof(esr_dvgo_bwd_t));return 0;}')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes == [ctypes.sizeof(_lib.EsrDvgo), _lib.EsrDvgo.n_samples.offset, _lib.EsrDvgo.near_.offset,
                     ctypes.sizeof(_lib.EsrDvgoRays), _lib.EsrDvgoRays.n_rays.offset, ctypes.sizeof(_lib.EsrDvgoOut),
                     ctypes.sizeof(_lib.EsrDvgoBwd)]
