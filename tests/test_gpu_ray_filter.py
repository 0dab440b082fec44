"""The training-ray filter on the MI355X (esr_nerf_amd/rayfilter.py over csrc/rayfilter.hip): flags bit-equal to the
reference-generated fixture (tests/golden/ray_filter.npz) for the coarse renderer and both branches of the fine one, first
hits against the retained torch path, the renderers' methods (chunk size, strides, ray counts), a ~200 k camera-ray set
against the float64 classifier of tests/ray_filter_ref.py, and the coarse trainer's set-up statements on the drop-in
classes."""
import numpy as np
import pytest
import torch

import ray_filter_ref as R
from conftest import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONFIGS = {"coarse_fixed": (0, True), "fine_fixed": (1, True), "fine_march": (1, False)}


@pytest.fixture(scope="module")
def models():
    return R.renderers(DEV)


def _rays(z):
    return torch.from_numpy(z["rays_o"]).to(DEV), torch.from_numpy(z["rays_d"]).to(DEV)


def _torch_first_hits(m, ro, rd, fixed):
    """Index of the first kept step per ray (-1: none) from the samplers and mask cache the retained torch path uses"""
    n = len(ro)
    if fixed:
        pts, out, _ = m.sample_ray_ori(ro, rd)
        inside = ~out
        inside[inside.clone()] = m.mask_cache(pts[inside])
        first = inside.to(torch.uint8).argmax(-1)
        return torch.where(inside.any(-1), first, torch.full_like(first, -1)).to(torch.int32)
    pts, ray_id, step_id = m.sample_ray(ro, rd)
    sel = m.mask_cache(pts)
    first = torch.full((n,), 1 << 30, dtype=torch.int64, device=ro.device)
    first.scatter_reduce_(0, ray_id[sel], step_id[sel], reduce="amin")
    return torch.where(first < (1 << 30), first, torch.full_like(first, -1)).to(torch.int32)


def test_kernel_flags_equal_the_reference_fixture(models):
    from esr_nerf_amd.rayfilter import filter_rays
    z = load_npz("ray_filter.npz")
    ro, rd = _rays(z)
    for key, (mi, fixed) in CONFIGS.items():
        keep = filter_rays(models[mi], ro, rd, fixed)
        assert keep.dtype == torch.bool and keep.shape == (len(ro),)
        diff = np.nonzero(keep.cpu().numpy() != z[f"keep/{key}"])[0]
        assert len(diff) == 0, (key, diff[:10], z["family"][diff[:10]])


def test_first_hits_equal_the_torch_path(models):
    from esr_nerf_amd.rayfilter import filter_rays
    z = load_npz("ray_filter.npz")
    ro, rd = _rays(z)
    for key, (mi, fixed) in CONFIGS.items():
        keep, first = filter_rays(models[mi], ro, rd, fixed, want_first_hit=True)
        want = _torch_first_hits(models[mi], ro, rd, fixed)
        assert first.dtype == torch.int32 and torch.equal(first, want), (key, int((first != want).sum()))
        assert torch.equal(keep, first >= 0)
        assert int((first >= 128).sum()) >= 3 and int(((first >= 64) & (first < 128)).sum()) >= 3     # later trips decide


def test_renderer_methods(models, capsys):
    from esr_nerf_amd.config import lts_cfg
    from esr_nerf_amd.esrnerf import ESRNeRF
    z = load_npz("ray_filter.npz")
    ro, rd = _rays(z)
    coarse, fine = models
    sc = R.slab()
    torch.manual_seed(0)
    np.random.seed(0)
    esr = ESRNeRF(lts_cfg(DEV, num_2ndrays=8, num_ltspts=12), sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min,
                  sc.mask_xyz_max, sc.mask_alpha_init, sc.mask_density, sc.s_val, sc.num_voxels)
    want = {k: torch.from_numpy(z[f"keep/{k}"]).to(DEV) for k in CONFIGS}
    assert torch.equal(coarse.filter_training_rays_in_maskcache_sampling(ro, rd, 4096), want["coarse_fixed"])
    out = capsys.readouterr().out
    assert "get_training_rays_in_maskcache_sampling: ratio" in out and "finish (eps time:" in out
    for m in (fine, esr):
        for rnd, key in ((True, "fine_fixed"), (False, "fine_march")):
            m.sdf_random_init = rnd
            for chunk in (1, 128, 10 ** 9):                                   # chunk_size does not touch device work
                assert torch.equal(m.filter_training_rays_in_maskcache_sampling(ro, rd, chunk), want[key]), (type(m), key, chunk)
            # the retained torch body gives the same flags (no ray of the fixture is marginal)
            assert torch.equal(m._filter_rays_torch(ro, rd, 256), want[key]), (type(m), key)
            # non-contiguous inputs: every other row of a larger buffer, and a transposed [3, n] buffer
            wide_o, wide_d = torch.zeros(2 * len(ro), 3, device=DEV), torch.ones(2 * len(ro), 3, device=DEV)
            wide_o[::2], wide_d[::2] = ro, rd
            assert not wide_o[::2].is_contiguous()
            assert torch.equal(m.filter_training_rays_in_maskcache_sampling(wide_o[::2], wide_d[::2], 128), want[key])
            assert torch.equal(m.filter_training_rays_in_maskcache_sampling(ro.t().contiguous().t(), rd.t().contiguous().t(), 128),
                               want[key])
            # ray counts: none, one, and counts that do not fill the last block's four waves
            for n in (0, 1, 2, 3, 5, 1001):
                got = m.filter_training_rays_in_maskcache_sampling(ro[:n], rd[:n], 128)
                assert got.shape == (n,) and torch.equal(got, want[key][:n]), (key, n)
    fine.sdf_random_init = True
    assert torch.equal(coarse._filter_rays_torch(ro, rd, 300), want["coarse_fixed"])


@pytest.mark.parametrize("fixed", [True, False])
def test_large_seeded_set_against_the_float64_classifier(models, fixed):
    from esr_nerf_amd.rayfilter import filter_rays
    fine = models[1]
    fine.sdf_random_init = fixed
    ro_h, rd_h = R.large_set()
    ro, rd = torch.from_numpy(ro_h).to(DEV), torch.from_numpy(rd_h).to(DEV)
    keep = filter_rays(fine, ro, rd, fixed)
    c = R.classify(R.scene_of(fine), ro_h, rd_h, fixed)
    bad, share = R.agreement(c["cls"], keep.cpu().numpy())
    print(f"fixed={fixed}: {len(ro_h)} rays, kept {int(keep.sum())}, marginal share {share:.5f}, firm mismatches {bad}")
    assert share <= R.MARGINAL_CAP, f"marginal share {share:.5f}"
    assert bad == 0, f"{bad} firm rays disagree with the float64 classifier (marginal share {share:.5f})"
    torch_keep = fine._filter_rays_torch(ro, rd, 16384)
    differ = (torch_keep != keep).cpu().numpy()
    firm_differ = int((differ & (c["cls"] != R.MARGINAL)).sum())
    print(f"   kernel vs torch path: {int(differ.sum())} rays differ, {firm_differ} of them firm")
    assert firm_differ == 0, f"{firm_differ} firm rays differ between the kernel and the torch path (marginal share {share:.5f})"
    fine.sdf_random_init = True


def test_coarse_setup_replay_and_one_training_step():
    """The statements of the reference's Coarse.load_model (app/coarse/coarse.py:189-215) on the drop-in classes, then one
    training step on the trimmed set."""
    import torch.nn.functional as F
    from esr_nerf_amd.config import coarse_cfg
    from esr_nerf_amd.data import BatchSampler
    from esr_nerf_amd.optimizer import create_optimizer_or_freeze_model
    from esr_nerf_amd.voxurfc import VoxurfC
    sc = R.slab()
    cfg = coarse_cfg(DEV, num_voxels=sc.num_voxels)
    cfg.system["data_preload"] = "cuda"
    torch.manual_seed(0)
    np.random.seed(0)
    renderer = VoxurfC(cfg, sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max, sc.mask_alpha_init,
                       sc.mask_density, cfg.app.trainer.s_start).to(DEV)
    optimizer = create_optimizer_or_freeze_model(renderer, sdf=0.1, off_color=0.1, off_rgbnet=1e-3, emo_color=0.1,
                                                 emo_rgbnet=1e-3)
    ro_h, rd_h = R.large_set(seed=9, side=64)
    g = torch.Generator().manual_seed(2)
    rd_t = torch.from_numpy(rd_h)
    data = dict(rays_o=torch.from_numpy(ro_h), rays_d=rd_t, viewdirs=rd_t / rd_t.norm(dim=-1, keepdim=True),
                rgbs=torch.rand(len(ro_h), 3, generator=g), em_modes=(torch.arange(len(ro_h)) % 2).long())
    keys = ["rgbs", "rays_o", "rays_d", "viewdirs", "em_modes"]
    mask = renderer.filter_training_rays_in_maskcache_sampling(data["rays_o"].to(DEV), data["rays_d"].to(DEV), 16384)
    assert mask.dtype == torch.bool and mask.device.type == "cuda" and 0 < int(mask.sum()) < len(mask)
    sampler = BatchSampler(cfg, data, keys, 1024)
    sampler.filter(mask)
    sampler.shuffle()
    kept_rows = set(mask.nonzero()[:, 0].tolist())
    assert sampler.data_num == len(kept_rows) and set(sampler.data_idxs.tolist()) == kept_rows
    renderer.train()
    before = {k: p.detach().clone() for k, p in renderer.named_parameters() if p.requires_grad}
    batch = sampler.sample()
    assert torch.equal(renderer.filter_training_rays_in_maskcache_sampling(batch["rays_o"], batch["rays_d"], 16384),
                       torch.ones(1024, dtype=torch.bool, device=DEV))          # only kept rays reach the step
    optimizer.zero_grad(set_to_none=True)
    res = renderer(rays_o=batch["rays_o"], rays_d=batch["rays_d"], viewdirs=batch["viewdirs"], em_modes=batch["em_modes"],
                   s_val=cfg.app.trainer.s_start)
    srgb = (res["srgb/rgb"] + res["etc/white_bg"] * 1.0).clamp(min=0.0, max=1.0)
    pout = res["etc/alphainv_cum"][..., -1].clamp(1e-6, 1 - 1e-6)
    loss = F.mse_loss(srgb, batch["rgbs"]) + cfg.app.trainer.weight_entropy_last * \
        -(pout * torch.log(pout) + (1 - pout) * torch.log(1 - pout)).mean()
    loss.backward()
    optimizer.step()
    assert bool(torch.isfinite(loss))
    moved = [k for k, p in renderer.named_parameters() if k in before and not torch.equal(p.detach(), before[k])]
    assert "sdf.grid" in moved and any(k.startswith("off_rgbnet") for k in moved), moved
