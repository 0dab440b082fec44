"""CPU side of the training-ray filter: the coarse renderer's two new methods against the reference-generated fixture
(tests/golden/ray_filter.npz, tools/gen_ray_filter_golden.py), the float64 classifier of tests/ray_filter_ref.py against the
reference's flags, the condition on the large seeded ray set the GPU test uses, and the C ABI's declaration."""
import os
import re

import numpy as np
import torch

import ray_filter_ref as R
from conftest import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"coarse_fixed": (0, True), "fine_fixed": (1, True), "fine_march": (1, False)}


def _fixture_and_models():
    z = load_npz("ray_filter.npz")
    models = R.renderers("cpu")
    assert str(z["scene"]) == R.SCENE and float(z["far"]) == float(np.float32(R.FAR))
    for m in models:
        assert list(m.sdf.grid.shape[2:]) == z["world_size"].tolist()
    return z, models


def test_coarse_sample_ray_ori_matches_reference():
    z, (coarse, _) = _fixture_and_models()
    pick = z["ori_rays"]
    ro, rd = torch.from_numpy(z["rays_o"][pick]), torch.from_numpy(z["rays_d"][pick])
    pts, mask, step = coarse.sample_ray_ori(ro, rd)
    assert pts.shape[1] == int(z["n_samples"])
    assert np.array_equal(pts.numpy(), z["ori_pts"], equal_nan=True)
    assert mask.dtype == torch.bool and np.array_equal(mask.numpy(), z["ori_mask"])
    assert np.array_equal(step.numpy(), z["ori_step"])
    assert 0 < z["ori_mask"].mean() < 1
    pts_t, _, step_t = coarse.sample_ray_ori(ro, rd, is_train=True)          # jittered: one offset in [0, 1) steps per ray
    off = (step_t / step[:, 1:2])[:, 0]
    assert step_t.shape == (len(pick), int(z["n_samples"])) and bool(((off >= 0) & (off < 1)).all()) and pts_t.shape == pts.shape


def test_coarse_filter_matches_reference_on_cpu(capsys):
    z, (coarse, _) = _fixture_and_models()
    ro, rd = torch.from_numpy(z["rays_o"]), torch.from_numpy(z["rays_d"])
    for chunk in (96, 5000):
        keep = coarse.filter_training_rays_in_maskcache_sampling(ro, rd, chunk)
        assert keep.dtype == torch.bool and np.array_equal(keep.numpy(), z["keep/coarse_fixed"])
    out = capsys.readouterr().out
    assert "get_training_rays_in_maskcache_sampling: ratio" in out and "finish (eps time:" in out


def test_fine_fixed_filter_matches_reference_on_cpu():
    """(the march branch's sampler is a library call on device tensors: tests/test_gpu_ray_filter.py)"""
    z, (_, fine) = _fixture_and_models()
    fine.sdf_random_init = True
    keep = fine.filter_training_rays_in_maskcache_sampling(torch.from_numpy(z["rays_o"]), torch.from_numpy(z["rays_d"]), 128)
    assert np.array_equal(keep.numpy(), z["keep/fine_fixed"])


def test_classifier_agrees_with_reference_and_fixture_has_no_marginal_ray():
    z, models = _fixture_and_models()
    for key, (mi, fixed) in CONFIGS.items():
        c = R.classify(R.scene_of(models[mi]), z["rays_o"], z["rays_d"], fixed)
        bad, share = R.agreement(c["cls"], z[f"keep/{key}"])
        assert share == 0.0 and bad == 0, (key, bad, share)
        assert np.array_equal(c["keep64"], z[f"keep/{key}"]), key
        # the families the kernel's trip loop needs: deciding trips beyond the first and the second
        assert (c["first64"] >= 128).sum() >= 3 and ((c["first64"] >= 64) & (c["first64"] < 128)).sum() >= 3, key
    assert (z["keep/fine_fixed"] != z["keep/fine_march"]).sum() >= 3          # far cuts the fixed sampler's t-range only


def test_large_set_marginal_share_is_within_the_cap():
    """A condition on the INPUTS of tests/test_gpu_ray_filter.py's large-set test, checked without a GPU"""
    _, (_, fine) = _fixture_and_models()
    ro, rd = R.large_set()
    assert 190_000 <= len(ro) <= 210_000
    S = R.scene_of(fine)
    for fixed in (True, False):
        c = R.classify(S, ro, rd, fixed)
        share = float((c["cls"] == R.MARGINAL).mean())
        kept = float((c["cls"] == R.KEEP).mean())
        assert share <= R.MARGINAL_CAP, (fixed, share)
        assert 0.1 < kept < 0.9, (fixed, kept)


def test_header_declares_esr_ray_filter_and_ctypes_agrees():
    from esr_nerf_amd import _lib, rayfilter
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    # the names only: tests/test_host.py checks every entry's restype and argument types against the header text
    assert "esr_ray_filter" in _lib.EXPORTS
    for name, val in (("ESR_RAY_FILTER_MARCH", rayfilter.MODE_MARCH), ("ESR_RAY_FILTER_FIXED", rayfilter.MODE_FIXED)):
        assert int(re.search(r"#define " + name + r" (\d+)", header).group(1)) == val
