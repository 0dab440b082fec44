"""The re-lighting edit-ray selection on the MI355X (esr_nerf_amd/relight.py over csrc/relight.hip): ``esr_mask_dilate`` bit
for bit against the numpy restatement (tests/relight_ref.py) and the reference-generated fixture
(tests/golden/edit_rays.npz), ``esr_edit_label`` against the reference's labels under the clear-ray rule of
tests/test_relight_host.py, the reference quirks by name, ``EditRaySelector`` and ``finetune_radiance`` on a slab scene."""
import os

import numpy as np
import pytest
import torch

import relight_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

Z = np.load(os.path.join(GOLDEN, "edit_rays.npz"), allow_pickle=False)
CASES = relight_ref.cases(Z)
LABELS = ("keep", "em_modes", "em_colors", "em_intensities")
UNCLEAR_CAP = 0.02


# ---- esr_mask_dilate -------------------------------------------------------------------------------------------------------
# the tile is 16 x 64: 70 exceeds it in both directions (and needs the > 64 KB LDS opt-in on this image), 200 exceeds the image
@pytest.mark.parametrize("ks,h,w,n_cond", [(1, 37, 53, 1), (2, 37, 53, 3), (3, 41, 29, 5), (10, 37, 53, 3), (11, 37, 53, 2),
                                           (10, 131, 67, 1), (40, 75, 131, 2), (70, 75, 131, 3), (200, 33, 47, 2), (5, 1, 1, 1),
                                           (10, 3, 200, 1), (9, 200, 3, 1)])
def test_dilation_is_bit_identical_to_the_definition(ks, h, w, n_cond):
    from esr_nerf_amd.relight import dilate_masks
    rng = np.random.default_rng(ks * 1000 + h)
    m = rng.random((n_cond, h, w)).astype(np.float32)
    m[rng.random((n_cond, h, w)) < 0.8] = 0.0                      # sparse: most windows see few positive pixels
    got = dilate_masks(torch.from_numpy(m).cuda(), ks)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == m.shape
    assert np.array_equal(got.cpu().numpy(), relight_ref.dilate(m, ks))


@pytest.mark.parametrize("name", CASES)
def test_dilation_equals_the_fixture(name):
    from esr_nerf_amd.relight import dilate_masks
    c = relight_ref.case(Z, name)
    assert np.array_equal(dilate_masks(c["em_masks"], int(c["ks"])).cpu().numpy(), c["dilated"])


def test_dilation_refuses_what_does_not_fit_with_an_error_code():
    from esr_nerf_amd.relight import dilate_masks
    m = torch.zeros(1, 600, 600, device="cuda")
    with pytest.raises(RuntimeError, match="code -2"):
        dilate_masks(m, 400)
    with pytest.raises(RuntimeError, match="code -1"):
        dilate_masks(m, 0)
    assert torch.equal(dilate_masks(m, 100), m)                   # the largest windows that fit still run


# ---- esr_edit_label ---------------------------------------------------------------------------------------------------------
def _label_case(c, **kw):
    from esr_nerf_amd.relight import label_edit_rays
    w, h = (int(x) for x in c["image_size"])
    out = label_edit_rays(torch.from_numpy(c["esp"]).cuda(), torch.from_numpy(c["pose"]), float(c["focal"]), w, h,
                          torch.from_numpy(c["dilated"]).cuda(), torch.from_numpy(c["em_modes_cond"]),
                          torch.from_numpy(c["em_intensities_cond"]), torch.from_numpy(c["em_colors_cond"]), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", [c for c in CASES if c != "integer"])
def test_labels_equal_the_references_on_every_clear_ray(name):
    delta = relight_ref.delta(Z)
    c = relight_ref.case(Z, name)
    r = relight_ref.case_label(c, np.float64)
    clear = r["clearance"] > delta
    got = _label_case(c, return_uv=True)
    fin = np.isfinite(r["uv"]).all(1)
    err = np.abs(got["uv"][fin].astype(np.float64) - r["uv"][fin]).max()
    print(f"{name}: delta {delta:.3e} px, {int((~clear).sum())} of {len(clear)} rays set aside, kernel |uv - float64| <= {err:.3e} px, "
          f"kept {int(got['keep'].sum())} (reference {int(c['keep'].sum())})")
    assert 1.0 - clear.mean() <= UNCLEAR_CAP
    # delta = 4 x the reference's error: the rule is sound while the kernel's own error stays under the remaining margin
    assert err <= delta / 2
    assert got["keep"].dtype == np.bool_ and got["em_modes"].dtype == np.int64 and got["em_colors"].shape == (len(clear), 2)
    for k in LABELS:
        assert np.array_equal(got[k][clear], c[k][clear]), k


def test_integer_coordinates_agree_with_the_reference_on_every_ray():
    """The projection is exact in float32 here, so only grid_sample's normalise / un-normalise round trip is exercised."""
    c = relight_ref.case(Z, "integer")
    got = _label_case(c, return_uv=True)
    assert np.array_equal(got["uv"], c["ref_uv"])
    for k in LABELS:
        bad = np.nonzero((got[k] != c[k]).reshape(len(c["keep"]), -1).any(1))[0]
        assert bad.size == 0, (k, bad[:10], c["ref_uv"][bad[:10]])


def test_two_runs_are_byte_identical():
    c = relight_ref.case(Z, "tall")
    a, b = _label_case(c, return_uv=True), _label_case(c, return_uv=True)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


F = 64.0
POSE = np.eye(4, dtype=np.float32)
POSE[:3, 3] = [2.0, -1.0, 3.0]


def _points_at(uv, w, h, depth=-2.0):
    """World points that project exactly onto ``uv`` under POSE and F (dyadic arithmetic: exact in float32)"""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    cam = np.stack([-(uv[:, 0] - (w / 2 - 0.5)) * depth / F, (uv[:, 1] - (h / 2 - 0.5)) * depth / F, np.full(len(uv), depth)], 1)
    return (cam + POSE[:3, 3].astype(np.float64)).astype(np.float32)


def _run(esp, w, h, masks, modes, intensities=None, colors=None, pose=POSE):
    from esr_nerf_amd.relight import label_edit_rays
    out = label_edit_rays(torch.from_numpy(np.asarray(esp, np.float32)).cuda(), torch.from_numpy(pose), F, w, h,
                          torch.from_numpy(np.asarray(masks, np.float32)).cuda(), modes, intensities, colors, return_uv=True)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("w,h", [(52, 40), (40, 52)])
def test_both_coordinates_are_tested_against_both_sizes(w, h):
    """pdra.py:997: with h < w a ray at u in (h - 1, w - 1] is out of bounds although it is inside the image, with h > w the
    same for v in (w - 1, h - 1]; the usable area is the square of the smaller size."""
    lo = min(w, h) - 1
    inside = [(3.0, 5.0), (lo, lo), (0.0, 0.0), (lo - 0.5, 2.0)]
    beyond = [(lo + 1.0, 5.0), (lo + 0.5, 5.0)] if w > h else [(5.0, lo + 1.0), (5.0, lo + 0.5)]
    outside = [(-1.0, 5.0), (5.0, -0.5), (max(w, h) + 2.0, 3.0)]
    uv = np.array(inside + beyond + outside)
    r = _run(_points_at(uv, w, h), w, h, np.ones((1, h, w)), [2], [1.5])
    assert np.array_equal(r["uv"], uv.astype(np.float32))
    assert r["keep"].tolist() == [True] * 4 + [False] * 5
    assert r["em_modes"].tolist() == [2] * 4 + [1] * 5 and r["em_intensities"].tolist() == [1.5] * 4 + [0.0] * 5


def test_a_later_condition_overrides_only_the_fields_it_sets():
    w, h = 52, 40
    esp = _points_at([(10.0, 10.0)], w, h)
    ones = lambda n: np.ones((n, h, w))
    col = [[0.2, 0.3, 0.9], [0.6, 0.7, 0.9], [0.4, 0.5, 0.9]]
    cases = [([2, 3], (3, 1.5, (0.6, 0.7))),            # i_change then c_change: the first one's intensity, the second's colour
             ([3, 2], (2, 2.5, (0.2, 0.3))),
             ([4, 0], (0, 0.0, (0.2, 0.3))),            # off resets the intensity and leaves the colour
             ([4, 1], (1, 1.5, (0.2, 0.3))),            # on sets the mode alone
             ([0, 4, 3], (3, 2.5, (0.4, 0.5)))]
    for modes, (mode, inten, colour) in cases:
        r = _run(esp, w, h, ones(len(modes)), modes, [1.5, 2.5, 3.5][:len(modes)], col[:len(modes)])
        assert r["keep"].tolist() == [True] and r["em_modes"].tolist() == [mode], modes
        assert r["em_intensities"].tolist() == [np.float32(inten)] and r["em_colors"].tolist() == [list(np.float32(colour))], modes
    # a condition whose mask misses the ray sets nothing
    masks = ones(2)
    masks[1] = 0.0
    r = _run(esp, w, h, masks, [2, 0], [1.5, 9.0])
    assert r["em_modes"].tolist() == [2] and r["em_intensities"].tolist() == [1.5]


def test_unmatched_and_out_of_bounds_rays_keep_the_defaults_and_absent_arrays_are_zeros():
    w, h = 52, 40
    masks = np.zeros((2, h, w))
    masks[1, 20:, :] = 0.5
    esp = _points_at([(10.0, 5.0), (10.0, 30.0), (-4.0, 30.0)], w, h)
    r = _run(esp, w, h, masks, [4, 4])
    assert r["keep"].tolist() == [False, True, False] and r["em_modes"].tolist() == [1, 4, 1]
    assert not r["em_colors"].any() and not r["em_intensities"].any()


def test_points_at_the_origin_are_projected_like_any_other_point():
    """A ray without a surviving sample has esp = (0, 0, 0) (eval_esp); the reference projects it (pdra.py:988-995)."""
    w, h = 52, 40
    pose = POSE.copy()
    pose[:3, 3] = [0.25, -0.125, 3.0]                                    # a camera that sees the origin
    want = relight_ref.project(np.zeros((1, 3), np.float32), np.linalg.inv(pose.astype(np.float64)), F, w, h)[0]
    assert 0 < want[0] < h - 1 and 0 < want[1] < h - 1, want
    r = _run(np.zeros((3, 3)), w, h, np.ones((1, h, w)), [0], pose=pose)
    assert np.abs(r["uv"] - want).max() < 1e-3
    assert r["keep"].tolist() == [True] * 3 and r["em_modes"].tolist() == [0] * 3


def test_non_finite_points_read_nothing_and_are_unselected():
    w, h = 52, 40
    nan, inf = float("nan"), float("inf")
    esp = np.array([[nan, 0, 0], [0, nan, 0], [0, 0, nan], [inf, 0, 0], [0, -inf, 0], [0, 0, inf], [inf, inf, inf],
                    [1e38, 1e38, -1e38], [nan, nan, nan]], np.float32)
    esp = np.concatenate([esp, _points_at([(10.0, 10.0)], w, h)])
    r = _run(esp, w, h, np.ones((2, h, w)), [4, 2], [1.5, 2.5], [[0.1, 0.2], [0.3, 0.4]])
    assert r["keep"].tolist() == [False] * 9 + [True]
    assert r["em_modes"].tolist() == [1] * 9 + [2]
    assert not r["em_colors"][:9].any() and not r["em_intensities"][:9].any()


# ---- EditRaySelector, finetune_radiance ----------------------------------------------------------------------------------
H, W, BATCH = 48, 40, 500


def _model_and_scene():
    from esr_nerf_amd.config import lts_cfg
    from esr_nerf_amd.esrnerf import ESRNeRF
    from esr_nerf_amd.synthetic import init_slab_model, slab_scene
    sc = slab_scene("g16", s_val=60.0, oblique=True, n_rays=H * W, seed=0)
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = lts_cfg("cuda:0", num_2ndrays=8, num_ltspts=12)
    cfg.system["data_preload"] = "cuda"
    m = init_slab_model(ESRNeRF(cfg, sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max,
                                sc.mask_alpha_init, sc.mask_density, sc.s_val, sc.num_voxels), sc)
    m.s_val = sc.s_val
    m.eval()
    return m, sc, cfg


KEYS = ["rgbs", "rays_o", "rays_d", "viewdirs", "em_modes"]


def _sampler(sc, cfg, bs=128):
    from esr_nerf_amd.data import RayGroupManager
    g = torch.Generator().manual_seed(5)
    perm = torch.randperm(H * W, generator=g)
    n_u = 1500
    return RayGroupManager(cfg, {k: sc.batch[k] for k in KEYS}, list(KEYS), bs, bs, uncert_data_idxs=perm[:n_u],
                           cert_data_idxs=perm[n_u:])


def _views(esp):
    """Two test views looking at the cloud of expected surface points from different sides, with overlapping conditions"""
    pts = esp.cpu().numpy().astype(np.float64)
    pts = pts[np.abs(pts).sum(1) > 0]
    centre, extent = pts.mean(0), np.abs(pts - pts.mean(0)).max()
    views = []
    for k, off in enumerate(([0.4, -0.5, 1.0], [-0.6, 0.3, 0.9])):
        eye = centre + 4.0 * extent * np.asarray(off) / np.linalg.norm(off)
        z = (eye - centre) / np.linalg.norm(eye - centre)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        P = np.eye(4)
        P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, np.cross(z, x), z, eye
        yy, xx = np.mgrid[0:H, 0:W]
        masks = np.stack([((yy - 20) ** 2 + (xx - 18) ** 2 <= 81) * 0.7, (np.abs(yy - 24 - 4 * k) <= 6) * (xx < 22) * 1.0,
                          (xx >= 30) * (yy < 12) * 0.4]).astype(np.float32)
        views.append(dict(poses=torch.from_numpy(P.astype(np.float32)), em_masks=torch.from_numpy(masks).reshape(-1),
                          em_modes=torch.tensor([2, 3, 0][k:] + [4][:k]), em_intensities=torch.tensor([1.5, 0.5, 2.0]),
                          em_colors=torch.tensor([[0.1, 0.9, 0.5], [0.6, 0.3, 0.5], [0.8, 0.8, 0.5]])))
    return views, 3.0 * W / 2        # focal length: the cloud (4 extents away) fills about a third of the width


def _state(s):
    return dict(u=s.uncert_data_idxs.clone(), c=s.cert_data_idxs.clone(), keys=list(s.keys),
                **{k: s.data[k].clone() for k in ("em_modes", "em_colors", "em_intensities")})


def _same_state(a, b):
    return a["keys"] == b["keys"] and all(torch.equal(a[k], b[k]) for k in a if k != "keys")


def test_selector_marches_once_and_applies_views_from_its_base_state():
    from esr_nerf_amd.relight import EditRaySelector
    m, sc, cfg = _model_and_scene()
    s = _sampler(sc, cfg)
    own_modes = s.data["em_modes"]
    base_u, base_c = s.uncert_data_idxs.clone(), s.cert_data_idxs.clone()
    m.train()
    sel = EditRaySelector(m, s, 1.0, (W, H), 10, BATCH)
    assert m.training                                                # the renderer's mode is put back
    m.eval()
    assert sel.esp.shape == (1500, 3) and torch.equal(sel.rows, base_u)
    for a in range(0, 1500, BATCH):                                  # the cache equals a fresh eval_esp per chunk
        rows = base_u[a:a + BATCH]
        fresh = m.eval_esp(**{k: s.data[k][rows] for k in ("rays_o", "rays_d", "viewdirs")})
        assert torch.equal(sel.esp[a:a + BATCH], fresh)
    views, focal = _views(sel.esp)
    sel.focal = focal
    got_a = sel.apply(views[0])
    assert got_a is s
    lab_a = {k: v.clone() for k, v in sel.labels.items()}
    st_a = _state(s)
    n_keep = int(lab_a["keep"].sum())
    print(f"view A keeps {n_keep} of 1500 rays, modes {torch.bincount(lab_a['em_modes'], minlength=5).tolist()}")
    assert 50 < n_keep < 1450 and len(torch.unique(lab_a["em_modes"])) >= 3
    assert s.keys == KEYS + ["em_colors", "em_intensities"]
    assert torch.equal(s.uncert_data_idxs, base_u[lab_a["keep"]])
    assert torch.equal(s.cert_data_idxs, torch.cat([base_c, base_u[~lab_a["keep"]]]))
    assert s.data["em_modes"] is not own_modes and torch.equal(own_modes, sc.batch["em_modes"].cuda())
    # what sample() carries: the labels of the rays it drew, zeros for the certain rows
    b = s.sample()
    nu = min(128, n_keep)
    for k in ("em_modes", "em_colors", "em_intensities"):
        assert torch.equal(b[k][:nu], lab_a[k][lab_a["keep"]][:nu]), k
        assert not b[k][nu:].any(), k
    assert torch.equal(b["rays_o"][:nu], s.data["rays_o"][base_u[lab_a["keep"]][:nu]])
    assert b["uncert_masks"][:nu].all() and not b["uncert_masks"][nu:].any()
    for _ in range(5):
        s.sample()                                                   # shuffles: the index vectors are permuted
    # A then B equals a fresh selector's B; B then A gives A again, byte for byte
    sel.apply(views[1])
    st_b = _state(s)
    assert not _same_state(st_a, st_b)
    s2 = _sampler(sc, cfg)
    sel2 = EditRaySelector(m, s2, focal, (W, H), 10, BATCH)
    assert torch.equal(sel2.esp, sel.esp)
    sel2.apply(views[1])
    assert _same_state(st_b, _state(s2))
    sel.apply(views[0])
    assert _same_state(st_a, _state(s))
    for k, v in sel.labels.items():
        assert torch.equal(v, lab_a[k]), k
    # the labels are the restatement's on every ray that is clear by 1e-3 px: float32 projection errors at these magnitudes
    # (coordinates of tens of pixels, points a few units from the camera) are of the order of 1e-5 px, as in the fixture
    c = views[0]
    masks = relight_ref.dilate(c["em_masks"].reshape(-1, H, W).numpy(), 10)
    r = relight_ref.label(sel.esp.cpu().numpy(), torch.inverse(c["poses"]).numpy(), focal, W, H, masks, c["em_modes"].numpy(),
                          c["em_intensities"].numpy(), c["em_colors"].numpy())
    clear = r["clearance"] > 1e-3
    assert clear.mean() > 0.98
    for k in LABELS:
        assert np.array_equal(lab_a[k].cpu().numpy()[clear], np.asarray(r[k])[clear]), k


def test_finetune_radiance_equals_driving_the_step_by_hand():
    from esr_nerf_amd.optimizer import create_optimizer_or_freeze_model
    from esr_nerf_amd.relight import EditRaySelector, finetune_radiance
    from esr_nerf_amd.trainer import FinetuneStep
    m, sc, cfg = _model_and_scene()
    s = _sampler(sc, cfg)
    sel = EditRaySelector(m, s, 1.0, (W, H), 10, BATCH)
    views, sel.focal = _views(sel.esp)
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    lrs, n_iters, weight = dict(emo_color=0.01, emo_rgbnet=1e-3), 4, 0.5

    def seed():
        torch.manual_seed(77)
        np.random.seed(77)

    seed()
    losses = finetune_radiance(m, sel, views[0], n_iters, lrs, weight, state=state)
    assert not m.training and len(losses) == n_iters and all(np.isfinite(losses)) and all(l > 0 for l in losses), losses
    after = {k: v.detach().clone() for k, v in m.state_dict().items()}
    changed = sorted(k for k in state if not torch.equal(state[k], after[k]))
    assert changed and all(k.startswith(("emo_color.", "emo_rgbnet.")) for k in changed), changed
    assert any(k.startswith("emo_color.") for k in changed) and any(k.startswith("emo_rgbnet.") for k in changed)
    assert [n for n, p in m.named_parameters() if p.requires_grad] == \
        [n for n, _ in m.named_parameters() if n.startswith(("emo_color.", "emo_rgbnet."))]

    # by hand: the same batches (the sampler from the selector's base state) and the same draws (the same generator state)
    m.load_state_dict(state, strict=False)
    assert all(torch.equal(state[k], v) for k, v in m.state_dict().items() if k in state)        # `state` restores them
    seed()
    sampler = sel.apply(views[0])
    opt = create_optimizer_or_freeze_model(m, **lrs)
    m.train(True, finetune=True)
    step, params, by_hand = FinetuneStep(m, weight=weight), dict(m.named_parameters()), []
    for _ in range(n_iters):
        batch = sampler.sample()
        opt.zero_grad(set_to_none=True)
        loss, grads = step.forward_loss_backward(batch, m.s_val)
        for name, g in grads.items():
            params[name].grad = g
        opt.step()
        by_hand.append(float(loss))
    m.eval()
    print("fine-tune losses", losses, "by hand", by_hand)
    assert losses == by_hand
    for k, v in m.state_dict().items():
        if k in after:
            assert torch.equal(v, after[k]), k
    # a second view through the same selector, with the checkpoint restored, starts from the same place
    seed()
    again = finetune_radiance(m, sel, views[0], n_iters, lrs, weight, state=state)
    assert again == losses
