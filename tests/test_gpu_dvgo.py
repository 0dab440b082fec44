"""The DVGO pre-stage on the HIP path (esr_nerf_amd/dvgo.py over csrc/dvgo.hip) against the torch restatement
tests/dvgo_ref.py (float32 sampling, float64 after it) and the reference's own DVGO (tests/golden/dvgo_small.npz):
sample decisions, the five training outputs and the grid gradients for every subset of upstream gradients, the seven
evaluation outputs, the view count, an empty batch, the alphamask loss and a short teacher-student training run."""
import itertools

import pytest
import torch

import dvgo_ref
from conftest import load_npz, rel_err
from esr_nerf_amd import optimizer
from esr_nerf_amd.config import alphamask_cfg
from esr_nerf_amd.dvgo import DVGO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAIN_KEYS = ("etc/alphainv_cum", "etc/weights", "etc/white_bg", "srgb/raw_rgb", "srgb/rgb")
EVAL_KEYS = ("etc/depth", "etc/disp", "etc/white_bg", "srgb/off_rgb", "srgb/on_rgb", "srgb/emo_rgb", "srgb/rgb")
GRIDS = ("density", "off_color", "emo_color")
FOUR = ("etc/alphainv_cum", "etc/weights", "srgb/raw_rgb", "srgb/rgb")


def make_model(num_voxels, lo, hi, near=0.2, far=6.0, stepsize=0.5, alpha_init=1e-6, grids=None):
    cfg = alphamask_cfg(DEV, num_voxels=num_voxels, stepsize=stepsize, alpha_init=alpha_init)
    m = DVGO(cfg, near, far, torch.tensor(lo, dtype=torch.float32, device=DEV),
             torch.tensor(hi, dtype=torch.float32, device=DEV)).to(DEV)
    if grids is not None:
        m.load_state_dict({k: v.float() for k, v in grids.items()})
    return m


def golden_case():
    z = load_npz("dvgo_small.npz")
    m = make_model(int(z["num_voxels"]), z["xyz_min"].tolist(), z["xyz_max"].tolist(), float(z["near"]), float(z["far"]),
                   float(z["stepsize"]), float(z["alpha_init"]), {k: torch.from_numpy(z[k]) for k in GRIDS})
    t = lambda k: torch.from_numpy(z[k]).to(DEV)
    return z, m, dict(rays_o=t("rays_o"), rays_d=t("rays_d"), em_modes=t("em_modes"), jitter=t("jitter"))


def random_grids(dims, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    X, Y, Z = dims
    coarse = torch.randn(1, 1, 9, 9, 9, generator=g, device=DEV) * 3 - 1
    density = torch.nn.functional.interpolate(coarse, size=(X, Y, Z), mode="trilinear", align_corners=True)
    density = density + 0.3 * torch.randn(1, 1, X, Y, Z, generator=g, device=DEV)
    density[..., : X // 5, :, :] = -100                                   # what maskout / cnt <= 2 write
    density[..., X // 2: X // 2 + 6, Y // 2: Y // 2 + 6, Z // 2: Z // 2 + 6] = 1e4     # 1 - alpha == 0
    cols = [torch.nn.functional.interpolate(torch.randn(1, 3, 9, 9, 9, generator=g, device=DEV) * 2, size=(X, Y, Z),
                                            mode="trilinear", align_corners=True) for _ in range(2)]
    return {"density": density, "off_color": cols[0], "emo_color": cols[1]}


def random_rays(n, lo, hi, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    lo, hi = torch.tensor(lo, device=DEV), torch.tensor(hi, device=DEV)
    c, r = (lo + hi) / 2, (hi - lo).norm() * 0.9
    src = torch.randn(n, 3, generator=g, device=DEV)
    src = c + src / src.norm(dim=-1, keepdim=True) * r
    tgt = lo + (hi - lo) * torch.rand(n, 3, generator=g, device=DEV)
    d = (tgt - src) * (0.3 + torch.rand(n, 1, generator=g, device=DEV))
    d[: n // 16, 1] = 0.0                                                  # exact zero components
    src[n // 16: n // 8] = lo + (hi - lo) * (0.3 + 0.4 * torch.rand(n // 16, 3, generator=g, device=DEV))  # inside
    em = (torch.rand(n, generator=g, device=DEV) < 0.5).long()
    jitter = torch.rand(n, 1, generator=g, device=DEV)
    return dict(rays_o=src.contiguous(), rays_d=d.contiguous(), em_modes=em, jitter=jitter)


def grids_of(m, dtype):
    return {k: getattr(m, k).detach().to(dtype).requires_grad_() for k in GRIDS}


def grid_grads(res, grids, up, keys):
    return torch.autograd.grad(sum((res[k] * up[k]).sum() for k in keys), [grids[k] for k in GRIDS], retain_graph=True,
                               allow_unused=True)


def check_training(m, b, seed=5):
    """outputs and grid gradients (for every subset of upstream gradients) at 1e-4 of the float64 restatement, or within
    3x torch float32's own distance from float64 where the reference's float32 arithmetic is coarser than that (alpha =
    1 - exp(-x) of a small x carries a few per cent of rounding in float32; at the reference size torch float32 itself
    is 3e-4 from float64 on alphainv_cum); the outputs also at 1e-5 of the float32 restatement"""
    res = m.render_training(b["rays_o"], b["rays_d"], b["em_modes"], b["jitter"])
    g64, g32 = grids_of(m, torch.float64), grids_of(m, torch.float32)
    r64 = dvgo_ref.training(m, g64, b["rays_o"], b["rays_d"], b["em_modes"], b["jitter"])
    r32 = dvgo_ref.training(m, g32, b["rays_o"], b["rays_d"], b["em_modes"], b["jitter"])
    for k in TRAIN_KEYS:
        assert res[k].shape == r64[k].shape, k
        assert rel_err(res[k], r64[k]) < max(1e-4, 3 * rel_err(r32[k], r64[k])), k
        assert rel_err(res[k], r32[k]) < 1e-5, k
    gen = torch.Generator(device=DEV).manual_seed(seed)
    up = {k: torch.randn(res[k].shape, generator=gen, device=DEV) for k in FOUR + ("etc/white_bg",)}
    subsets = [s for n in (1, 2, 4) for s in itertools.combinations(FOUR, n)] + [("etc/white_bg", "srgb/rgb")]
    for keys in subsets:
        got = grid_grads(res, {k: getattr(m, k) for k in GRIDS}, up, keys)
        want = grid_grads(r64, g64, {k: v.double() for k, v in up.items()}, keys)
        base = grid_grads(r32, g32, up, keys)
        for k, a, w, f in zip(GRIDS, got, want, base):
            if w is None:
                assert a is None or not a.any(), (keys, k)
                continue
            assert torch.isfinite(a).all(), (keys, k)
            bar = max(1e-4, 3 * rel_err(f, w))
            assert rel_err(a, w) < bar, (keys, k, rel_err(a, w), bar)
    return res


def check_eval(m, b):
    for mode in (0, 1):
        with torch.no_grad():
            got = m.eval()(rays_o=b["rays_o"], rays_d=b["rays_d"], em_modes=mode)
            want = dvgo_ref.evaluate(m, grids_of(m, torch.float64), b["rays_o"], b["rays_d"], mode)
            base = dvgo_ref.evaluate(m, grids_of(m, torch.float32), b["rays_o"], b["rays_d"], mode)
        assert set(got) == set(EVAL_KEYS)
        for k in EVAL_KEYS:
            assert got[k].shape == want[k].shape, (mode, k)
            assert rel_err(got[k], want[k]) < max(1e-4, 3 * rel_err(base[k], want[k])), (mode, k)
    m.train()


def test_golden_case_against_the_reference_and_the_restatement():
    z, m, b = golden_case()
    res = check_training(m, b)
    for k in TRAIN_KEYS:
        assert rel_err(res[k], torch.from_numpy(z["train/" + k])) < 1e-4, k
    up = {k: torch.from_numpy(z["up/" + k]).to(DEV) for k in FOUR}
    for k, g in zip(GRIDS, grid_grads(res, {k: getattr(m, k) for k in GRIDS}, up, FOUR)):
        assert torch.isfinite(g).all()
        assert rel_err(g, torch.from_numpy(z["grad/" + k])) < 2e-3, k      # the golden's own float32 error: host test
    check_eval(m, b)
    for mode in (0, 1):
        with torch.no_grad():
            ev = m.eval()(rays_o=b["rays_o"], rays_d=b["rays_d"], em_modes=mode)
        for k in EVAL_KEYS:
            assert rel_err(ev[k], torch.from_numpy(z[f"eval{mode}/{k}"])) < 1e-4, (mode, k)


def test_reference_size_case():
    lo, hi = [-1.2, -1.0, -0.9], [1.1, 1.3, 0.8]
    m = make_model(1024000, lo, hi)
    m.load_state_dict(random_grids(tuple(m.density.shape[2:]), 11))
    assert m.N_samples > 300
    b = random_rays(8192, lo, hi, 12)
    res = check_training(m, b, seed=13)
    assert (res["etc/white_bg"] == 0).any()                          # behind the clamped cluster
    check_eval(m, dict(b, rays_o=b["rays_o"][:2048], rays_d=b["rays_d"][:2048]))


def test_sample_decisions_equal_torch_float32():
    """with a positive density everywhere, a sample's alpha is 0 exactly when it is out of the box: the kernel's zero
    weights are torch's float32 out-of-box mask; the colours (looked up at every sample) agree with torch's float32
    lookups at the float32 points to float32 rounding"""
    lo, hi = [-1.2, -1.0, -0.9], [1.1, 1.3, 0.8]
    m = make_model(200000, lo, hi, alpha_init=0.01)
    g = random_grids(tuple(m.density.shape[2:]), 21)
    g["density"] = g["density"].abs().clamp(max=3.0) * 0.1
    m.load_state_dict(g)
    b = random_rays(4096, lo, hi, 22)
    with torch.no_grad():
        res = m.render_training(b["rays_o"], b["rays_d"], b["em_modes"], b["jitter"])
        pts, out = dvgo_ref.sample(m, b["rays_o"], b["rays_d"], m.N_samples, b["jitter"])
        raw = torch.sigmoid(m.grid_sampler(pts, m.off_color)) + (b["em_modes"] == 1).float()[:, None, None] * \
            torch.sigmoid(m.grid_sampler(pts, m.emo_color))
    assert out.any() and (~out).any()
    assert torch.equal(res["etc/weights"] == 0, out)
    assert (res["srgb/raw_rgb"] - raw).abs().max() < 1e-5


def test_empty_batch():
    _, m, b = golden_case()
    e = {k: v[:0] for k, v in b.items()}
    res = m.render_training(e["rays_o"], e["rays_d"], e["em_modes"], e["jitter"])
    S = m.N_samples
    shapes = {"etc/alphainv_cum": (0, S + 1), "etc/weights": (0, S), "etc/white_bg": (0, 1), "srgb/raw_rgb": (0, S, 3),
              "srgb/rgb": (0, 3)}
    for k, s in shapes.items():
        assert tuple(res[k].shape) == s, k
    sum(v.sum() for v in res.values()).backward()
    assert not m.density.grad.any()
    with torch.no_grad():
        ev = m.eval()(rays_o=e["rays_o"], rays_d=e["rays_d"], em_modes=1)
    assert all(v.shape[0] == 0 for v in ev.values())


def test_alphamask_loss_gradients_match_the_golden():
    z, m, b = golden_case()
    res = m.render_training(b["rays_o"], b["rays_d"], b["em_modes"], b["jitter"])
    loss = dvgo_ref.alphamask_loss(res, torch.from_numpy(z["rgbs"]).to(DEV))
    loss.backward()
    assert float(loss.detach()) == pytest.approx(float(z["loss"]), rel=1e-5)
    for k in GRIDS:
        g = getattr(m, k).grad
        assert torch.isfinite(g).all()
        assert rel_err(g, torch.from_numpy(z["loss_grad/" + k])) < 2e-3, k


def test_count_views_golden():
    z, m, _ = golden_case()
    vo, vd = torch.from_numpy(z["views_o"]).to(DEV), torch.from_numpy(z["views_d"]).to(DEV)
    got = m.voxel_count_views(vo, vd, 50)
    want, sums = dvgo_ref.count_views(m, vo, vd, tuple(m.density.shape[2:]))
    near_one = ((sums - 1).abs() < 1e-5).any(0)[None, None]
    assert got.shape == m.density.shape and got.dtype == torch.float32
    assert torch.equal(got[~near_one], want[~near_one])
    assert torch.equal(got[~near_one].cpu(), torch.from_numpy(z["count"])[~near_one.cpu()])


def test_count_views_reference_size():
    lo, hi = [-1.2, -1.0, -0.9], [1.1, 1.3, 0.8]
    m = make_model(1024000, lo, hi)
    g = torch.Generator(device=DEV).manual_seed(40)
    lo_t, hi_t = torch.tensor(lo, device=DEV), torch.tensor(hi, device=DEV)
    vo, vd = [], []
    for v in range(3):                                                    # one camera per view, 64 x 64 rays into the box
        cam = (lo_t + hi_t) / 2 + torch.nn.functional.normalize(torch.randn(3, generator=g, device=DEV), dim=0) * 2.5
        tgt = lo_t + (hi_t - lo_t) * torch.rand(64 * 64, 3, generator=g, device=DEV)
        vo.append(cam.expand(64 * 64, 3))
        vd.append(tgt - cam)
    vo, vd = torch.stack(vo).contiguous(), torch.stack(vd).contiguous()
    got = m.voxel_count_views(vo, vd, 8192)
    want, sums = dvgo_ref.count_views(m, vo, vd, tuple(m.density.shape[2:]))
    # at ~100 cells per axis the float32 grid index carries ~1e-5 of rounding into every trilinear weight (torch's
    # float32 sums are as far from float64 as the kernel's): the band around 1 is 1e-4 here
    near_one = ((sums - 1).abs() < 1e-4).any(0)[None, None]
    assert near_one.sum() < 1000 and (want > 0).sum() > 10000
    assert torch.equal(got[~near_one], want[~near_one])


def test_count_views_lattice_aligned():
    """box [0, 8]^3 at 729 voxels: index == world coordinate, and a step of exactly one voxel (stepsize 1.125 *
    voxel_size 8/9 rounds to 1.0): axis rays through lattice lines put every sample on a node, so per-view sums are
    integers, many exactly 1 -- the kernel's count must equal the float64 one on every voxel"""
    m = make_model(729, [0.0, 0.0, 0.0], [8.0, 8.0, 8.0], near=0.0, far=100.0, stepsize=1.125)
    assert m.world_size.tolist() == [9, 9, 9]
    yz = torch.stack(torch.meshgrid(torch.arange(9.0), torch.arange(9.0), indexing="ij"), -1).reshape(-1, 2).to(DEV)
    n = len(yz)
    o1 = torch.cat([torch.full((n, 1), -2.0, device=DEV), yz], 1)                     # along +x
    o2 = torch.cat([yz[:, :1], torch.full((n, 1), 11.0, device=DEV), yz[:, 1:]], 1)  # along -y
    d1 = torch.tensor([[1.0, 0.0, 0.0]], device=DEV).expand(n, 3)
    d2 = torch.tensor([[0.0, -1.0, 0.0]], device=DEV).expand(n, 3)
    # each view: every line once, the first half of them twice
    vo = torch.stack([torch.cat([o1, o1[: n // 2]]), torch.cat([o2, o2[: n // 2]])]).contiguous()
    vd = torch.stack([torch.cat([d1, d1[: n // 2]]), torch.cat([d2, d2[: n // 2]])]).contiguous()
    got = m.voxel_count_views(vo, vd, 100)
    want, sums = dvgo_ref.count_views(m, vo, vd, (9, 9, 9))
    assert ((sums == 1).sum() > 100) and ((sums == 2).sum() > 100)
    assert torch.equal(got, want)


class _Grids(torch.nn.Module):
    """the three grids as named parameters, for the float32 restatement's optimizer"""

    def __init__(self, m):
        super().__init__()
        for k in GRIDS:
            setattr(self, k, torch.nn.Parameter(getattr(m, k).detach().clone()))


def _psnr(a, b):
    return float(-10 * torch.log10(((a - b) ** 2).mean()))


def test_teacher_student_training_matches_the_float32_restatement():
    """a student from zeros learns a smooth teacher for 300 steps with optimizer.Adam + set_pervoxel_lr, once on the
    drop-in and once on the float32 torch restatement, with identical batches and jitter: final PSNRs within 0.1 dB"""
    lo, hi = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
    teacher = make_model(32768, lo, hi, alpha_init=1e-4)
    g = random_grids(tuple(teacher.density.shape[2:]), 31)
    g["density"] = (g["density"] * 2 + 6).clamp(-20, 20)
    teacher.load_state_dict(g)
    pool = random_rays(65536, lo, hi, 32)
    with torch.no_grad():
        t = dvgo_ref.training(teacher, grids_of(teacher, torch.float32), pool["rays_o"], pool["rays_d"],
                              pool["em_modes"], torch.full_like(pool["jitter"], 0.5))
        target = (t["srgb/rgb"] + t["etc/white_bg"]).clamp(0, 1)
    student = make_model(32768, lo, hi, alpha_init=1e-4)
    shadow = _Grids(student)
    cnt = torch.ones_like(student.density.detach())
    cnt[..., :4, :, :] = 0.5
    lrs = dict(density=0.1, off_color=0.1, emo_color=0.1)
    opts = []
    for model in (student, shadow):
        o = optimizer.create_optimizer_or_freeze_model(model, **lrs)
        o.set_pervoxel_lr(cnt)
        opts.append(o)
    gen = torch.Generator(device=DEV).manual_seed(33)
    decay = 0.1 ** (1 / 20000)
    for step in range(300):
        idx = torch.randint(0, len(target), (2048,), generator=gen, device=DEV)
        jit = torch.rand(2048, 1, generator=gen, device=DEV)
        b = {k: v[idx] for k, v in pool.items()}
        for model, o in zip((student, shadow), opts):
            o.zero_grad(set_to_none=True)
            if model is student:
                res = student.render_training(b["rays_o"], b["rays_d"], b["em_modes"], jit)
            else:
                res = dvgo_ref.training(student, {k: getattr(shadow, k) for k in GRIDS}, b["rays_o"], b["rays_d"],
                                        b["em_modes"], jit)
            dvgo_ref.alphamask_loss(res, target[idx]).backward()
            o.step()
            for group in o.param_groups:
                group["lr"] *= decay
    with torch.no_grad():
        ev = slice(0, 8192)
        psnr = []
        for grids in ({k: getattr(student, k) for k in GRIDS}, {k: getattr(shadow, k) for k in GRIDS}):
            r = dvgo_ref.training(student, grids, pool["rays_o"][ev], pool["rays_d"][ev], pool["em_modes"][ev],
                                  torch.full_like(pool["jitter"][ev], 0.5))
            psnr.append(_psnr((r["srgb/rgb"] + r["etc/white_bg"]).clamp(0, 1), target[ev]))
    start = _psnr(torch.ones_like(target[ev]), target[ev])
    assert psnr[1] > start + 1, (start, psnr)
    assert abs(psnr[0] - psnr[1]) < 0.1, psnr
