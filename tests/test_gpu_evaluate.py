"""The view loop of esr_nerf_amd/evaluate.py on the MI355X, on the small slab scenes: ``render_view`` against one
``forward_evaluate`` call on all rays, ``postprocess_view`` + ``view_metrics`` against the numpy restatement
(tests/metrics_ref.py) applied to the downloaded images, ``evaluate_views`` over views of both emissive modes, and the
memory bound that separates ``render_view`` from a list-append + ``torch.cat``."""
import numpy as np
import pytest
import torch

import metrics_ref
from conftest import rel_err

pytestmark = pytest.mark.gpu

H, W, BATCH = 48, 40, 500                      # 1920 rays: three full chunks and one of 420
TOL = 1e-4                                     # the project's parity bar


def _scene(name="g16", seed=0):
    from esr_nerf_amd.synthetic import slab_scene
    return slab_scene(name, s_val=60.0, oblique=True, n_rays=H * W, seed=seed)


def _renderer(kind, sc):
    from esr_nerf_amd.synthetic import init_slab_model
    torch.manual_seed(0)
    np.random.seed(0)
    box = (sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max, sc.mask_alpha_init, sc.mask_density)
    if kind == "VoxurfF":
        from esr_nerf_amd.config import fine_cfg
        from esr_nerf_amd.voxurff import VoxurfF
        m = init_slab_model(VoxurfF(fine_cfg("cuda:0"), *box, sc.s_val, sc.num_voxels), sc)
    elif kind == "ESRNeRF":
        from esr_nerf_amd.config import lts_cfg
        from esr_nerf_amd.esrnerf import ESRNeRF
        m = init_slab_model(ESRNeRF(lts_cfg("cuda:0", num_2ndrays=8, num_ltspts=12), *box, sc.s_val, sc.num_voxels), sc)
    else:
        from esr_nerf_amd.config import coarse_cfg
        from esr_nerf_amd.voxurfc import VoxurfC
        m = init_slab_model(VoxurfC(coarse_cfg("cuda:0", num_voxels=sc.num_voxels), *box, sc.s_val), sc)
    m.s_val = sc.s_val
    m.eval()
    return m


def _rays(sc):
    return {k: sc.batch[k].cuda() for k in ("rays_o", "rays_d", "viewdirs")}


EXTRA = {"VoxurfF": {}, "VoxurfC": {}, "ESRNeRF": dict(render_pbr=False, chunk_sz=4096)}


@pytest.mark.parametrize("kind", ["VoxurfF", "ESRNeRF", "VoxurfC"])
def test_render_view_matches_one_call_on_all_rays(kind):
    from esr_nerf_amd.evaluate import render_view
    sc = _scene()
    m, b, pos = _renderer(kind, sc), _rays(sc), torch.eye(3).cuda()
    whole = m(em_modes=1, pos_rt=pos, **b, **EXTRA[kind])
    got = render_view(m, b["rays_o"], b["rays_d"], b["viewdirs"], 1, pos, H, W, BATCH, **EXTRA[kind])
    assert list(got) == list(whole)
    for k, v in whole.items():
        want = v.reshape(H, W, -1).squeeze(-1)
        assert got[k].shape == want.shape and got[k].dtype == want.dtype and got[k].is_cuda, k
        e = rel_err(got[k], want)
        assert e <= TOL, (k, e)


def test_render_view_refuses_a_ray_count_that_is_not_the_view():
    from esr_nerf_amd.evaluate import render_view
    sc = _scene()
    b = _rays(sc)
    with pytest.raises(ValueError):
        render_view(None, b["rays_o"][:100], b["rays_d"][:100], b["viewdirs"][:100], 1, torch.eye(3).cuda(), H, W, BATCH)


def test_render_view_holds_one_set_of_output_buffers():
    """Peak memory of the chunk loop <= the output buffers + the peak of ONE single-chunk forward_evaluate + one chunk's
    outputs.  A list of chunk results plus torch.cat holds the outputs twice and exceeds it."""
    from esr_nerf_amd.evaluate import render_view
    sc = _scene()
    m, b, pos = _renderer("VoxurfF", sc), _rays(sc), torch.eye(3).cuda()
    batch = 200                                                # small chunks: the buffers outweigh one call's working set
    chunk = {k: v[:batch] for k, v in b.items()}
    for _ in range(2):                                         # warm: packed weights, allocator pools
        out = m(em_modes=1, pos_rt=pos, **chunk)
    torch.cuda.synchronize()
    chunk_bytes = sum(v.numel() * v.element_size() for v in out.values())
    del out
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = m(em_modes=1, pos_rt=pos, **chunk)
    torch.cuda.synchronize()
    one_call = torch.cuda.max_memory_allocated() - base
    del out
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = render_view(m, b["rays_o"], b["rays_d"], b["viewdirs"], 1, pos, H, W, batch)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    buf_bytes = sum(v.numel() * v.element_size() for v in res.values())
    slack = 512 * (len(res) + 8)                               # the allocator rounds every block up to 512 B
    print(f"buffers {buf_bytes} B, one chunk call {one_call} B, one chunk's outputs {chunk_bytes} B, loop peak {peak} B")
    assert peak <= buf_bytes + one_call + chunk_bytes + slack
    # the bound separates the loop from cat at this size: cat holds the outputs twice, 2 x buffers, which is above it
    assert 2 * buf_bytes > buf_bytes + one_call + chunk_bytes + slack


def _targets(seed):
    g = torch.Generator().manual_seed(seed)
    rgbs = torch.rand(H * W, 3, generator=g)
    hdrs = torch.rand(H * W, 3, generator=g) * 1.5
    areas = torch.rand(H * W, generator=g) > 0.5
    return rgbs, hdrs, areas


def test_postprocess_and_view_metrics_match_the_restatement():
    from esr_nerf_amd.evaluate import postprocess_view, render_view, view_metrics
    sc = _scene()
    m, b, pos = _renderer("VoxurfF", sc), _rays(sc), torch.eye(3).cuda()
    raw = render_view(m, b["rays_o"], b["rays_d"], b["viewdirs"], 1, pos, H, W, BATCH)
    raw["lin/rgb"] = raw["lin/rgb"] * 3.0 - 0.1                # reach both clamps of the lin/ branch
    rgbs, hdrs, _ = _targets(0)
    host = {k: v.cpu().numpy() for k, v in raw.items()}
    post = postprocess_view(raw, True, want_u8=True)
    wbg = np.clip(host["etc/white_bg"], 0, 1) if list(raw).index("etc/white_bg") == 0 else host["etc/white_bg"]
    assert set(post) == set(raw) | {k + "_gamma" for k in raw if k.startswith("lin/")}
    for k, v in host.items():
        if k == "etc/white_bg":
            want, c01 = metrics_ref.post_image(v)
        else:
            first = list(raw).index(k) < list(raw).index("etc/white_bg")
            want, c01 = metrics_ref.post_image(v, host["etc/white_bg"] if first else np.clip(host["etc/white_bg"], 0, 1), 1.0,
                                               lin=k.startswith("lin/"))
        assert np.array_equal(post[k].cpu().numpy(), want), k
        assert np.array_equal(post.u8[k].cpu().numpy(), metrics_ref.to_u8(post[k].cpu().numpy())), k
        if k.startswith("lin/"):
            g = metrics_ref.apply_gamma_curve(c01)
            assert np.abs(post[k + "_gamma"].cpu().numpy() - g).max() <= 1e-6 * max(1.0, np.abs(g).max()), k
    assert float(post["lin/rgb"].max()) > 1.0 and float(post["lin/rgb_gamma"].max()) <= 1.0 + 1e-6
    R, Hd = rgbs.reshape(H, W, 3), hdrs.reshape(H, W, 3)
    for fused in (False, True):
        p = postprocess_view(raw, True, rgbs=R.cuda(), hdrs=Hd.cuda()) if fused else post
        assert bool(p.sqerr) == fused
        got = view_metrics(p, R.cuda(), hdrs=Hd.cuda(), em_mode=1)
        assert list(got) == ["lin/MSE_EXR_off", "lin/MSE_EXR_on", "srgb/MSE", "srgb/PSNR", "srgb/SSIM", "lin/MSE", "lin/PSNR",
                             "lin/SSIM"]
        img = {k: p[k].cpu().numpy() for k in ("srgb/rgb", "lin/rgb", "lin/rgb_gamma")}
        want = {"lin/MSE_EXR_on": metrics_ref.sqerr_sum(img["lin/rgb"], Hd.numpy()) / (H * W * 3),
                "srgb/MSE": metrics_ref.sqerr_sum(img["srgb/rgb"], R.numpy()) / (H * W * 3),
                "lin/MSE": metrics_ref.sqerr_sum(img["lin/rgb_gamma"], R.numpy()) / (H * W * 3)}
        assert got["lin/MSE_EXR_off"] is None
        for k, w in want.items():
            assert abs(got[k] - w) <= 1e-12 * w, (k, fused)
        for space, key in (("srgb", "srgb/rgb"), ("lin", "lin/rgb_gamma")):
            assert got[f"{space}/PSNR"] == pytest.approx(metrics_ref.loss2psnr(want[f"{space}/MSE"]), abs=1e-9)
            assert abs(got[f"{space}/SSIM"] - metrics_ref.rgb_ssim(img[key], R.numpy(), 1)) <= 1e-10, space


def test_evaluate_views_over_both_emissive_modes():
    from esr_nerf_amd.evaluate import evaluate_views, postprocess_view, render_view
    from esr_nerf_amd import metrics
    sc = _scene()
    m, pos = _renderer("ESRNeRF", sc), torch.eye(3)
    views = []
    for i, em in enumerate((0, 1)):
        s = _scene(seed=i)
        rgbs, hdrs, areas = _targets(10 + i)
        views.append(dict(rays_o=s.batch["rays_o"], rays_d=s.batch["rays_d"], viewdirs=s.batch["viewdirs"], em_mode=em,
                          pos_rt=pos, rgbs=rgbs, hdrs=hdrs, areas=areas))
    k_val = 0.05
    out = evaluate_views(m, views, BATCH, True, H, W, k_val=k_val, return_images=True, render_pbr=False, chunk_sz=4096)
    mt = out["metrics"]
    assert set(mt) == {"lin/MSE_EXR_off", "lin/MSE_EXR_on", "srgb/MSE", "srgb/PSNR", "srgb/SSIM", "lin/MSE", "lin/PSNR",
                       "lin/SSIM"}
    assert all(len(v) == 2 for v in mt.values())
    assert mt["lin/MSE_EXR_off"][1] is None and mt["lin/MSE_EXR_on"][0] is None
    assert mt["lin/MSE_EXR_off"][0] is not None and mt["lin/MSE_EXR_on"][1] is not None
    assert out["mean"]["lin/MSE_EXR_off"] == mt["lin/MSE_EXR_off"][0]
    assert out["mean"]["srgb/SSIM"] == pytest.approx(np.mean(mt["srgb/SSIM"]), abs=1e-15)
    # the pooled IoU against the counts of each view's own mask
    inter = union = 0
    for v in views:
        d = {k: v[k].cuda() for k in ("rays_o", "rays_d", "viewdirs")}
        raw = render_view(m, d["rays_o"], d["rays_d"], d["viewdirs"], v["em_mode"], pos.cuda(), H, W, BATCH, render_pbr=False,
                          chunk_sz=4096)
        mask = (raw["lin/emit"] > k_val).any(-1).cpu().numpy()
        _, i, u = metrics_ref.iou(mask, v["areas"].reshape(H, W).numpy())
        inter, union = inter + i, union + (mask | v["areas"].reshape(H, W).numpy()).sum()
    assert out["scene"]["etc/IoU"] == inter / max(1, union)
    imgs = out["images"]
    assert imgs["target"][0].dtype == np.uint8 and imgs["srgb/rgb"][1].shape == (H, W, 3) and "lin/rgb_gamma" in imgs
    assert all(len(v) == 2 for v in imgs.values())
