"""Stage hand-over kernels on the MI355X (esr_nerf_amd/csrc/gridsetup.hip, esr_nerf_amd/gridsetup.py) against the float64
restatement of tests/setup_ref64.py: the resample per value at K_RESAMPLE, the max pool bit for bit, the mask and the bounds
node by node outside the decision band; then the wiring (DenseGrid.scale_volume_grid, set_nonempty_mask, fine_from_coarse,
coarse_from_alphamask) on GPU models against the same calls on CPU copies.

Every test prints the figure it asserts (run with -s to see them).
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import setup_ref64 as R
from conftest import load_npz

pytestmark = pytest.mark.gpu

GUARD = 64                      # guard floats before and after a kernel's output
SENTINEL = -12345.5


def _lib():
    from esr_nerf_amd import _lib as L
    return L


def _raw_resample(v, size, in_off=0, out_off=0):
    """esr_grid_resample through raw pointers: the input at float offset in_off of its buffer, the output at out_off + GUARD
    of a sentinel-filled one.  Returns (out, guards untouched, input unchanged)"""
    L = _lib()
    X, Y, Z, ch = v.shape
    n_out = size[0] * size[1] * size[2] * ch
    src = torch.full((v.size + in_off + 8,), 7.25, dtype=torch.float32, device="cuda")
    src[in_off:in_off + v.size] = torch.from_numpy(v).reshape(-1).cuda()
    before = src.clone()
    buf = torch.full((n_out + 2 * GUARD + out_off,), SENTINEL, dtype=torch.float32, device="cuda")
    rc = L.lib().esr_grid_resample(C.c_void_p(src.data_ptr() + 4 * in_off), X, Y, Z, ch,
                                   C.c_void_p(buf.data_ptr() + 4 * (GUARD + out_off)), *size, L.stream_ptr("cuda:0"))
    assert rc == 0
    torch.cuda.synchronize()
    lo, hi = GUARD + out_off, GUARD + out_off + n_out
    guards_ok = bool((buf[:lo] == SENTINEL).all()) and bool((buf[hi:] == SENTINEL).all())
    return buf[lo:hi].reshape(*size, ch).cpu().numpy(), guards_ok, torch.equal(src, before)


# ---- resample -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.RESAMPLE_CASES, ids=[R.case_id(c) for c in R.RESAMPLE_CASES])
def test_resample_per_value(case):
    from esr_nerf_amd.gridsetup import resample_grid
    v = R.resample_input(case)
    ref, absref = R.resample_ref(v, case[1])
    got, guards_ok, input_ok = _raw_resample(v, case[1])
    ratio = R.resample_ratio(got, ref, absref)
    print(f"\n[resample {R.case_id(case)}] worst |gpu - ref| / (U absref) = {ratio:.4g} (K_RESAMPLE = {R.K_RESAMPLE})")
    assert ratio <= R.K_RESAMPLE
    assert guards_ok and input_ok
    if case[0] == case[1]:
        assert np.array_equal(got, v)                                        # identity size: bit-equal to the input
    # the Python entry: the same bytes, on a second run as well
    view = torch.from_numpy(v).cuda()
    view = view[..., 0].contiguous() if case[2] == 1 else view
    a, b = resample_grid(view, case[1]), resample_grid(view, case[1])
    assert tuple(a.shape) == (*case[1], *view.shape[3:]) and torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy().reshape(got.shape), got)


@pytest.mark.parametrize("ch,in_off,out_off", [(1, 1, 0), (1, 0, 1), (1, 1, 3), (6, 6, 0), (6, 0, 6), (6, 6, 6)])
def test_resample_unaligned_pointers(ch, in_off, out_off):
    """in and out 4 bytes (C = 1) and one 24-byte record (C = 6) off the allocator's alignment: the same values"""
    case = ((5, 7, 3), (13, 9, 4), ch)
    v = R.resample_input(case)
    base, ok0, _ = _raw_resample(v, case[1])
    got, guards_ok, input_ok = _raw_resample(v, case[1], in_off, out_off)
    assert ok0 and guards_ok and input_ok
    assert np.array_equal(got, base)


# ---- max pool -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES, ids=str)
def test_maxpool_bit_equal_to_torch(shape):
    from esr_nerf_amd.gridsetup import maxpool3d
    v = R.maxpool_input(shape)
    dev = torch.from_numpy(v).cuda()[None, None]
    for ks in R.MAXPOOL_KS:
        want = F.max_pool3d(torch.from_numpy(v)[None, None], kernel_size=ks, padding=ks // 2, stride=1)
        got = maxpool3d(dev, ks)
        assert got.shape == want.shape and got.is_contiguous()
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.numpy().view(np.uint32)), ks
    assert np.array_equal(dev.cpu().numpy()[0, 0].view(np.uint32), v.view(np.uint32))          # input untouched
    with pytest.raises(NotImplementedError):
        maxpool3d(dev, 4)


# ---- mask ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.MASK_CASES))
def test_nonempty_mask_outside_the_band(name):
    from esr_nerf_amd.gridsetup import nonempty_mask
    shape, box, _, _ = R.MASK_CASES[name]
    axes = [torch.linspace(float(np.float32(box[a])), float(np.float32(box[3 + a])), shape[a], device="cuda") for a in range(3)]
    inp = R.mask_input(name, [a.cpu().numpy() for a in axes])
    alpha, band = R.node_alpha(inp["pooled"], inp["box"], R.ACT_SHIFT, inp["axes"])
    dec, firm = R.decide(alpha, band, R.THRES, strict=False)
    pooled = torch.from_numpy(inp["pooled"]).cuda()[None, None]
    g = torch.Generator().manual_seed(1)
    sdf0 = torch.randn(1, 1, *shape, generator=g)
    sdf = sdf0.cuda()
    mask, count = nonempty_mask(pooled, inp["box"], R.ACT_SHIFT, R.THRES, axes, sdf=sdf)
    torch.cuda.synchronize()
    m = mask.cpu().numpy()
    print(f"\n[mask {name}] true {int(m.sum())} of {m.size}, band nodes {int((~firm).sum())}, differ inside band "
          f"{int((m != dec)[~firm].sum())}")
    assert mask.dtype == torch.bool and tuple(mask.shape) == shape
    assert np.array_equal(m[firm], dec[firm])
    assert int(count) == int(m.sum())
    got = sdf.cpu()[0, 0].numpy()
    assert (got[~m] == 1.0).all()
    assert np.array_equal(got[m].view(np.uint32), sdf0[0, 0].numpy()[m].view(np.uint32))
    if "outside" in name:
        assert not m[0, 0, 0] and not m[-1, -1, -1]                      # zero padding outside the mask box
    # mask only: the same decisions, the SDF left alone
    keep = sdf.clone()
    mask2, count2 = nonempty_mask(pooled, inp["box"], R.ACT_SHIFT, R.THRES, axes)
    assert torch.equal(mask2, mask) and int(count2) == int(count) and torch.equal(sdf, keep)


# ---- bounds -------------------------------------------------------------------------------------------------------------------
def _raw_bounds(density, box):
    from esr_nerf_amd.gridsetup import bounds_axes
    L = _lib()
    d = torch.from_numpy(density).cuda()
    lo, hi = torch.tensor(box[:3], device="cuda"), torch.tensor(box[3:], device="cuda")
    axes = bounds_axes(lo, hi, density.shape)
    part = torch.empty(L.DENSITY_BOUNDS_BLOCKS * 6, dtype=torch.float32, device="cuda")
    out = torch.full((6,), 3.0, dtype=torch.float32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    rc = L.lib().esr_density_bounds(L.ptr(d), *density.shape, (C.c_float * 6)(*box), R.ACT_SHIFT, R.THRES,
                                    *[L.ptr(a) for a in axes], L.ptr(part), L.ptr(out), L.ptr(count), L.stream_ptr("cuda:0"))
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(count), [a.cpu().numpy() for a in axes]


@pytest.mark.parametrize("name", list(R.BOUNDS_CASES))
def test_density_bounds(name):
    from esr_nerf_amd.gridsetup import density_bounds
    density = R.bounds_density(name)
    out, count, axes = _raw_bounds(density, R.MASK_BOX)
    ref = R.bounds_ref(density, R.MASK_BOX, R.ACT_SHIFT, R.THRES, axes)
    print(f"\n[bounds {name}] count {count} (firm {ref['count_lo']}, band {ref['n_band']}), box {out.tolist()}")
    assert ref["count_lo"] <= count <= ref["count_hi"]
    for slot in range(6):
        assert float(out[slot]) in ref["allowed"][slot], (slot, float(out[slot]), ref["allowed"][slot])
    dev = torch.from_numpy(density).cuda()[None, None]
    box = (torch.tensor(R.MASK_BOX[:3]), torch.tensor(R.MASK_BOX[3:]))
    if name == "nothing":
        assert count == 0 and (out[:3] == np.inf).all() and (out[3:] == -np.inf).all()
        with pytest.raises(ValueError):
            density_bounds(dev, box, R.ACT_SHIFT, R.THRES)
    else:
        lo, hi = density_bounds(dev, box, R.ACT_SHIFT, R.THRES)
        assert lo.is_cuda and np.array_equal(torch.cat([lo, hi]).cpu().numpy(), out)


# ---- wiring -------------------------------------------------------------------------------------------------------------------
def _fine_pair():
    """the same small fine model on the GPU and on the CPU (the CPU copy runs the torch lines the renderers keep)"""
    from esr_nerf_amd.config import fine_cfg
    from esr_nerf_amd.synthetic import init_slab_model, slab_scene
    from esr_nerf_amd.voxurff import VoxurfF
    sc = slab_scene("g16", mask="prune")
    models = []
    for dev in ("cuda:0", "cpu"):
        torch.manual_seed(0)
        np.random.seed(0)
        m = VoxurfF(fine_cfg(dev), sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max,
                    sc.mask_alpha_init, sc.mask_density, sc.s_val, sc.num_voxels)
        models.append(m)
    init_slab_model(models[0], sc)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        models[0].off_color.grid.copy_(torch.randn(models[0].off_color.grid.shape, generator=g).cuda())
        models[0].sdf.grid.copy_((torch.randn(models[0].sdf.grid.shape, generator=g) * 0.3).cuda())
    models[1].load_state_dict({k: v.cpu() for k, v in models[0].state_dict().items()})
    return models[0], models[1], sc


def _mask_check(m_gpu, m_cpu, what):
    """both models' non-empty masks against the restatement: equal outside the band"""
    mc = m_gpu.mask_cache
    shape = tuple(m_gpu.sdf.grid.shape[2:])
    axes = [torch.linspace(float(m_gpu.xyz_min[i]), float(m_gpu.xyz_max[i]), shape[i], device="cuda").cpu().numpy()
            for i in range(3)]
    box = [*mc.xyz_min.tolist(), *mc.xyz_max.tolist()]
    alpha, band = R.node_alpha(mc.density[0, 0].cpu().numpy(), box, mc.act_shift, axes)
    dec, firm = R.decide(alpha, band, mc.mask_cache_thres, strict=False)
    g, c = m_gpu.nonempty_mask[0, 0].cpu().numpy(), m_cpu.nonempty_mask[0, 0].numpy()
    print(f"\n[{what}] mask true {int(g.sum())} of {g.size}, band nodes {int((~firm).sum())}, gpu/cpu differ {int((g != c).sum())}")
    assert m_gpu.nonempty_mask.dtype == torch.bool and tuple(m_gpu.nonempty_mask.shape) == (1, 1, *shape)
    assert np.array_equal(g[firm], dec[firm]) and np.array_equal(c[firm], dec[firm])
    return g, c, firm


def test_models_agree_at_construction_and_after_scale_volume_grid():
    m_gpu, m_cpu, sc = _fine_pair()
    assert torch.equal(m_gpu.mask_cache.density.cpu(), m_cpu.mask_cache.density)        # esr_maxpool3d against F.max_pool3d
    before = {k: getattr(m_gpu, k).device_view().cpu().numpy() for k in ("sdf", "off_color", "emo_color")}
    for m in (m_gpu, m_cpu):
        m.scale_volume_grid(sc.num_voxels * 4)
    size = tuple(m_gpu._world_size_l)
    assert size == tuple(m_cpu._world_size_l) and size != before["sdf"].shape
    g, c, firm = _mask_check(m_gpu, m_cpu, "scale_volume_grid")
    for k in ("sdf", "off_color", "emo_color"):
        grid = getattr(m_gpu, k).grid
        assert tuple(grid.shape) == (1, getattr(m_gpu, k).channels, *size) and isinstance(grid, torch.nn.Parameter)
        if k != "sdf":
            assert grid.is_contiguous(memory_format=torch.channels_last_3d)
        ref, absref = R.resample_ref(before[k], size)
        for m, mask, K in ((m_gpu, g, R.K_RESAMPLE), (m_cpu, c, R.K_RESAMPLE_CAP)):
            got = getattr(m, k).device_view().cpu().numpy()
            if k == "sdf":                         # pinned to 1 outside the mask, the resampled value inside
                assert (got[~mask] == 1.0).all()
                ratio = R.resample_ratio(got[mask], ref[mask], absref[mask])
            else:
                ratio = R.resample_ratio(got, ref, absref)
            print(f"[scale_volume_grid {k} on {m.sdf.grid.device}] worst ratio {ratio:.4g}")
            assert ratio <= K, (k, ratio)


def _gauss64(vol, w):
    """Conv3d(1, 1, k, padding=k // 2, padding_mode="replicate") in float64"""
    k = w.shape[0]
    p = np.pad(vol, k // 2, mode="edge")
    X, Y, Z = vol.shape
    out = np.zeros_like(vol)
    for a in range(k):
        for b in range(k):
            for c in range(k):
                out += w[a, b, c] * p[a:a + X, b:b + Y, c:c + Z]
    return out


def test_fine_from_coarse_on_the_gpu_and_on_a_cpu_copy():
    """coarse SDF / sdf_reduce -> resample -> 5^3 Gaussian.  Bound per value: the resample's K U absref carried through the
    (positive) Gaussian weights, plus the 125 accumulations of the convolution itself, each at most U of the running
    sum of |w| |v| (first order): (K + 126) U gauss(absref)."""
    from esr_nerf_amd import checkpoint
    from esr_nerf_amd.config import coarse_cfg, fine_cfg
    from esr_nerf_amd.modules import Gaussian3DConv
    from esr_nerf_amd.synthetic import slab_scene
    from esr_nerf_amd.voxurfc import VoxurfC
    from esr_nerf_amd.voxurff import VoxurfF
    sc = slab_scene("g16", mask="prune")
    torch.manual_seed(0)
    np.random.seed(0)
    vc = VoxurfC(coarse_cfg("cuda:0", num_voxels=sc.num_voxels // 3), sc.near, sc.far, sc.xyz_min, sc.xyz_max,
                 sc.mask_xyz_min, sc.mask_xyz_max, sc.mask_alpha_init, sc.mask_density, sc.s_val)
    rec = checkpoint.renderer_record(vc)
    rec_cpu = dict(rec, params={k: v.cpu() for k, v in rec["params"].items()},
                   **{k: rec[k].cpu() for k in ("xyz_min", "xyz_max", "mask_xyz_min", "mask_xyz_max", "mask_density")})
    m_gpu = checkpoint.fine_from_coarse(VoxurfF, fine_cfg("cuda:0"), rec, "cuda:0", sc.num_voxels, sdf_reduce=0.3)
    m_cpu = checkpoint.fine_from_coarse(VoxurfF, fine_cfg("cpu"), rec_cpu, "cpu", sc.num_voxels, sdf_reduce=0.3)
    size = tuple(m_gpu._world_size_l)
    coarse = (rec_cpu["params"]["sdf.grid"] / 0.3)[0, 0].numpy()
    assert coarse.shape != size
    ref, absref = R.resample_ref(coarse, size)
    w = Gaussian3DConv(ksize=5, sigma=1).m.weight.detach()[0, 0].double().numpy()
    ref, absref = _gauss64(ref, w), _gauss64(absref, w)
    g, c, _ = _mask_check(m_gpu, m_cpu, "fine_from_coarse")
    for m, mask, K in ((m_gpu, g, R.K_RESAMPLE), (m_cpu, c, R.K_RESAMPLE_CAP)):
        got = m.sdf.grid.detach()[0, 0].cpu().numpy()
        assert (got[~mask] == 1.0).all()
        ratio = R.resample_ratio(got[mask], ref[mask], absref[mask])
        print(f"[fine_from_coarse sdf on {m.sdf.grid.device}] worst ratio {ratio:.4g} (bound {K + 126})")
        assert ratio <= K + 126
    assert m_gpu.sdf_random_init is False


def test_coarse_from_alphamask_against_the_golden():
    from esr_nerf_amd import checkpoint
    from esr_nerf_amd.config import coarse_cfg
    from esr_nerf_amd.voxurfc import VoxurfC
    z = load_npz("stage_setup.npz")
    cfg = SimpleNamespace(app=SimpleNamespace(model=SimpleNamespace(alpha_init=float(z["am/alpha_init"]))))
    rec = dict(cfg=cfg, near=float(z["am/near"]), far=float(z["am/far"]), xyz_min=torch.from_numpy(z["am/xyz_min"]),
               xyz_max=torch.from_numpy(z["am/xyz_max"]), params={"density": torch.from_numpy(z["am/density"])})
    lo, hi = checkpoint.alphamask_bounds(rec["params"]["density"].cuda(), rec["xyz_min"].cuda(), rec["xyz_max"].cuda(),
                                         float(z["am/alpha_init"]), float(z["am/bbox_thres"]))
    # (the golden's density has no band node: tests/test_grid_setup_host.py::test_bounds_restatement_against_golden)
    assert np.array_equal(lo.cpu().numpy(), z["am/bbox_min"]) and np.array_equal(hi.cpu().numpy(), z["am/bbox_max"])
    m = checkpoint.coarse_from_alphamask(VoxurfC, coarse_cfg("cuda:0", num_voxels=4000), rec, "cuda:0",
                                         float(z["am/bbox_thres"]), float(z["am/world_bound_scale"]), 0.2)
    assert isinstance(m, VoxurfC) and m.sdf.grid.is_cuda
    assert np.array_equal(m.xyz_min.cpu().numpy(), z["am/wide_min"]) and np.array_equal(m.xyz_max.cpu().numpy(), z["am/wide_max"])
    assert np.array_equal(m.mask_xyz_min.cpu().numpy(), z["am/xyz_min"])
    assert np.array_equal(m.mask_cache.density.cpu().numpy(), z["mc/pooled"])           # esr_maxpool3d, the reference's pool
    assert bool(m.nonempty_mask.any()) and not bool(m.nonempty_mask.all())
    assert bool((m.sdf.grid[~m.nonempty_mask] == 1).all())
