"""CPU checks of the stage hand-over (esr_nerf_amd/gridsetup.py, csrc/gridsetup.hip): the float64 restatement of
tests/setup_ref64.py against torch and against the reference's recorded results, the binary32 emulation and its mutants,
the band census of every mask and bounds input, the ABI, and ``checkpoint.coarse_from_alphamask`` on a CPU record."""
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import setup_ref64 as R
from conftest import ROOT, load_npz

CASE_IDS = [R.case_id(c) for c in R.RESAMPLE_CASES]


def _interpolate(v, size):
    t = torch.from_numpy(v).permute(3, 0, 1, 2)[None].contiguous()
    return F.interpolate(t, size=size, mode="trilinear", align_corners=True)[0].permute(1, 2, 3, 0).numpy()


@pytest.fixture(scope="module")
def golden():
    return load_npz("stage_setup.npz")


# ---- resample -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.RESAMPLE_CASES, ids=CASE_IDS)
def test_resample_restatement_against_interpolate(case):
    v = R.resample_input(case)
    ref, absref = R.resample_ref(v, case[1])
    ratio = R.resample_ratio(_interpolate(v, case[1]), ref, absref)
    print(f"\n[{R.case_id(case)}] F.interpolate: worst |torch - ref| / (U absref) = {ratio:.3g}")
    assert ratio <= R.K_RESAMPLE_CAP
    if case[0] == case[1]:
        assert np.array_equal(ref.astype(np.float32), v)            # the identity size copies the grid


@pytest.mark.parametrize("case", R.RESAMPLE_CASES, ids=CASE_IDS)
def test_resample_emulation_inside_the_first_order_bound(case):
    v = R.resample_input(case)
    ref, absref = R.resample_ref(v, case[1])
    ratio = R.resample_ratio(R.resample_emul(v, case[1]), ref, absref)
    assert ratio <= R.K_RESAMPLE_CAP, ratio
    if case[0] == case[1]:
        assert np.array_equal(R.resample_emul(v, case[1]), v)


@pytest.mark.parametrize("mutant", ["align_corners_false", "i1_unclamped", "round_half", "swap_xz"])
def test_resample_mutants_are_rejected(mutant):
    rejected = []
    for case in R.RESAMPLE_CASES:
        v = R.resample_input(case)
        ref, absref = R.resample_ref(v, case[1])
        rejected.append(R.resample_ratio(R.resample_emul(v, case[1], mutant), ref, absref) > R.K_RESAMPLE_CAP)
    # (an identity-size case cannot see a coordinate mutant; the read past the grid's end shows on every case)
    general = [r for r, c in zip(rejected, R.RESAMPLE_CASES) if c[0] != c[1]]
    assert all(general), list(zip(CASE_IDS, rejected))
    if mutant == "i1_unclamped":
        assert all(rejected)


def test_resample_golden(golden):
    """the reference's own DenseGrid.scale_volume_grid (recorded) sits inside the bound of the restatement"""
    for ch in (1, 6):
        v = golden[f"up/c{ch}/in"]
        ref, absref = R.resample_ref(v, (13, 9, 4))
        assert R.resample_ratio(np.moveaxis(golden[f"up/c{ch}/out"][0], 0, -1), ref, absref) <= R.K_RESAMPLE_CAP


def test_k_resample_follows_the_measurement():
    assert R.MEASURED_RESAMPLE, "K_RESAMPLE is committed next to the worst ratios measured on the MI355X"
    assert set(R.MEASURED_RESAMPLE) == set(CASE_IDS)
    worst = max(R.MEASURED_RESAMPLE.values())
    assert R.K_RESAMPLE == math.floor(worst) + 1 <= R.K_RESAMPLE_CAP


# ---- max pool -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES, ids=str)
@pytest.mark.parametrize("ks", R.MAXPOOL_KS)
def test_maxpool_restatement_against_torch(shape, ks):
    v = R.maxpool_input(shape)
    want = F.max_pool3d(torch.from_numpy(v)[None, None], kernel_size=ks, padding=ks // 2, stride=1)[0, 0].numpy()
    assert np.array_equal(R.maxpool_ref(v, ks), want)
    if ks > 1 and v.size > 100:                 # (in the tiny volumes the +inf cell fills every window)
        assert not np.array_equal(R.maxpool_ref(v, ks, pad_value=0.0), want)        # the zero-padding mutant


# ---- mask and bounds ----------------------------------------------------------------------------------------------------------
def _torch_mask(pooled, box, thres, axes):
    """MaskCache.forward + the node coordinates of set_nonempty_mask (the torch lines the renderers keep)"""
    from esr_nerf_amd.modules import MaskCache
    mc = MaskCache(torch.tensor(box[:3]), torch.tensor(box[3:]), torch.zeros(1, 1, 1, 1, 1), R.ALPHA_INIT, thres, 1)
    mc.density = torch.from_numpy(pooled)[None, None]
    pts = torch.stack(torch.meshgrid(*[torch.from_numpy(a) for a in axes], indexing="ij"), -1)
    return mc(pts).numpy()


@pytest.mark.parametrize("name", list(R.MASK_CASES))
def test_mask_restatement_against_torch(name):
    inp = R.mask_input(name)
    alpha, band = R.node_alpha(inp["pooled"], inp["box"], R.ACT_SHIFT, inp["axes"])
    dec, firm = R.decide(alpha, band, R.THRES, strict=False)
    got = _torch_mask(inp["pooled"], inp["box"], R.THRES, inp["axes"])
    assert np.array_equal(got[firm], dec[firm])
    if "outside" in name:                         # zero padding: a node outside the mask box sees alpha_init < thres
        lo, hi = inp["box"][:3], inp["box"][3:]
        out = np.zeros(inp["sdf_shape"], bool)
        for a in range(3):
            sh = [1, 1, 1]
            sh[a] = -1
            ax = inp["axes"][a].reshape(sh)
            step = (hi[a] - lo[a]) / (inp["pooled"].shape[a] - 1)
            out |= (ax < lo[a] - step) | (ax > hi[a] + step)
        assert out.any() and not dec[out].any()


def test_mask_golden(golden):
    """the reference's own MaskCache (recorded): pooled density bit-equal, decisions equal outside the band"""
    dens = golden["am/density"][0, 0]
    assert np.array_equal(R.maxpool_ref(dens, int(golden["mc/ks"])), golden["mc/pooled"][0, 0])
    for name in R.MASK_CASES:
        if f"mc/{name}/mask" not in golden:
            continue
        shape, box, _, _ = R.MASK_CASES[name]
        axes = [R.linspace32(box[a], box[3 + a], shape[a]) for a in range(3)]
        alpha, band = R.node_alpha(golden["mc/pooled"][0, 0], R.MASK_BOX, R.ACT_SHIFT, axes)
        dec, firm = R.decide(alpha, band, R.THRES, strict=False)
        assert (~firm).sum() <= 2
        assert np.array_equal(golden[f"mc/{name}/mask"][firm], dec[firm])


def test_threshold_is_inclusive_for_the_mask():
    """a node made to sit exactly on thres: ``>=`` keeps it, the ``>`` mutant drops it (and nothing else moves)"""
    inp = R.mask_input("inside-19x16x12")
    alpha, _ = R.node_alpha(inp["pooled"], inp["box"], R.ACT_SHIFT, inp["axes"])
    cell = np.unravel_index(np.argmin(np.abs(alpha - R.THRES)), alpha.shape)
    thres = float(alpha.astype(np.float32)[cell])
    keep = R.mask_emul(inp["pooled"], inp["box"], R.ACT_SHIFT, thres, inp["axes"])
    mutant = R.mask_emul(inp["pooled"], inp["box"], R.ACT_SHIFT, thres, inp["axes"], strict=True)
    assert keep[cell] and not mutant[cell]
    assert (keep != mutant).sum() == 1


def test_band_census():
    """a condition on the inputs, not a measurement: at most 2 nodes per case may be decided either way"""
    for name in R.MASK_CASES:
        inp = R.mask_input(name)
        alpha, band = R.node_alpha(inp["pooled"], inp["box"], R.ACT_SHIFT, inp["axes"])
        n_band = int((~R.decide(alpha, band, R.THRES, strict=False)[1]).sum())
        print(f"\n[mask {name}] band nodes: {n_band} of {alpha.size}")
        assert n_band <= 2, name
    for name in R.BOUNDS_CASES:
        d = R.bounds_density(name)
        ref = R.bounds_ref(d, R.MASK_BOX, R.ACT_SHIFT, R.THRES, R.bounds_axes32(R.MASK_BOX, d.shape))
        print(f"[bounds {name}] band nodes: {ref['n_band']} of {d.size}, active {ref['count_lo']}")
        assert ref["n_band"] <= 2, name


def test_bounds_restatement_against_golden(golden):
    d = golden["am/density"][0, 0]
    ref = R.bounds_ref(d, R.MASK_BOX, R.ACT_SHIFT, float(golden["am/bbox_thres"]), R.bounds_axes32(R.MASK_BOX, d.shape))
    assert ref["count_lo"] <= int(golden["am/active"]) <= ref["count_hi"]
    got = np.concatenate([golden["am/bbox_min"], golden["am/bbox_max"]])
    for slot in range(6):
        assert float(got[slot]) in ref["allowed"][slot], slot


def test_bounds_cases_cover_the_extremes():
    for name, want in (("one-cell", 1), ("corners", 2), ("nothing", 0)):
        d = R.bounds_density(name)
        axes = R.bounds_axes32(R.MASK_BOX, d.shape)
        ref = R.bounds_ref(d, R.MASK_BOX, R.ACT_SHIFT, R.THRES, axes)
        assert ref["count_lo"] == ref["count_hi"] == want
    assert ref["allowed"][0] == {math.inf} and ref["allowed"][3] == {-math.inf}
    d = R.bounds_density("corners")
    axes = R.bounds_axes32(R.MASK_BOX, d.shape)
    ref = R.bounds_ref(d, R.MASK_BOX, R.ACT_SHIFT, R.THRES, axes)
    assert [next(iter(s)) for s in ref["allowed"]] == [float(axes[a][0]) for a in range(3)] + [float(axes[a][-1]) for a in range(3)]


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("esr_grid_resample", "esr_maxpool3d", "esr_nonempty_mask", "esr_density_bounds")


def test_new_entries_are_declared_exported_and_typed():
    from esr_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert name in _lib.EXPORTS and name in _lib.SIGNATURES
    assert int(re.search(r"#define ESR_RESAMPLE_MAX_C (\d+)", header).group(1)) == _lib.RESAMPLE_MAX_C
    assert int(re.search(r"#define ESR_DENSITY_BOUNDS_BLOCKS (\d+)", header).group(1)) == _lib.DENSITY_BOUNDS_BLOCKS


def test_entries_refuse_bad_arguments_before_any_launch():
    """argument errors return ESR_EINVAL with no device work (NULL pointers, sizes < 1, C outside 1..16, even ks)"""
    import ctypes as C
    from esr_nerf_amd import _lib, build
    build.build_lib()
    L = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    box = (C.c_float * 6)(-1, -1, -1, 1, 1, 1)
    assert L.esr_grid_resample(None, 2, 2, 2, 1, p, 2, 2, 2, None) == -1
    assert L.esr_grid_resample(p, 2, 2, 2, 0, p, 2, 2, 2, None) == -1
    assert L.esr_grid_resample(p, 2, 2, 2, 17, p, 2, 2, 2, None) == -1
    assert L.esr_grid_resample(p, 2, 0, 2, 1, p, 2, 2, 2, None) == -1
    assert L.esr_grid_resample(p, 2, 2, 2, 1, p, 2, 2, 0, None) == -1
    assert L.esr_grid_resample(C.c_void_p(p.value + 2), 2, 2, 2, 1, p, 2, 2, 2, None) == -1
    for ks in (0, 2, 4, 9, -1):
        assert L.esr_maxpool3d(p, 2, 2, 2, ks, p, None) == -1
    assert L.esr_maxpool3d(p, 2, 2, 0, 3, p, None) == -1
    assert L.esr_maxpool3d(None, 2, 2, 2, 3, p, None) == -1
    assert L.esr_nonempty_mask(p, 2, 2, 2, box, 0.0, 0.5, p, p, None, 2, 2, 2, None, p, p, None) == -1
    assert L.esr_nonempty_mask(p, 2, 2, 2, box, 0.0, 0.5, p, p, p, 2, 2, 2, None, None, p, None) == -1
    assert L.esr_nonempty_mask(p, 2, 2, 2, box, 0.0, 0.5, p, p, p, 2, 0, 2, None, p, p, None) == -1
    assert L.esr_nonempty_mask(p, 2, 2, 2, None, 0.0, 0.5, p, p, p, 2, 2, 2, None, p, p, None) == -1
    assert L.esr_density_bounds(p, 2, 2, 2, box, 0.0, 0.5, p, p, p, None, p, p, None) == -1
    assert L.esr_density_bounds(p, 0, 2, 2, box, 0.0, 0.5, p, p, p, p, p, p, None) == -1
    assert L.esr_density_bounds(p, 2, 2, 2, box, 0.0, 0.5, p, p, p, p, p, None, None) == -1


def test_python_wrappers_refuse_cpu_tensors():
    from esr_nerf_amd import gridsetup
    with pytest.raises(RuntimeError, match="no CPU kernel"):
        gridsetup.resample_grid(torch.zeros(2, 2, 2), (3, 3, 3))
    with pytest.raises(RuntimeError, match="no CPU kernel"):
        gridsetup.maxpool3d(torch.zeros(1, 1, 2, 2, 2), 3)
    with pytest.raises(RuntimeError, match="no CPU kernel"):
        gridsetup.density_bounds(torch.zeros(1, 1, 2, 2, 2), (torch.zeros(3), torch.ones(3)), 0.0, 0.5)


# ---- the alphamask -> coarse hand-off -----------------------------------------------------------------------------------------
def _alphamask_record(golden):
    cfg = SimpleNamespace(app=SimpleNamespace(model=SimpleNamespace(alpha_init=float(golden["am/alpha_init"]))))
    return dict(cfg=cfg, near=float(golden["am/near"]), far=float(golden["am/far"]),
                xyz_min=torch.from_numpy(golden["am/xyz_min"]), xyz_max=torch.from_numpy(golden["am/xyz_max"]),
                params={"density": torch.from_numpy(golden["am/density"])})


def test_coarse_from_alphamask_on_a_cpu_record(golden):
    from esr_nerf_amd import checkpoint
    from esr_nerf_amd.config import coarse_cfg
    from esr_nerf_amd.voxurfc import VoxurfC
    rec = _alphamask_record(golden)
    lo, hi = checkpoint.alphamask_bounds(rec["params"]["density"], rec["xyz_min"], rec["xyz_max"],
                                         float(golden["am/alpha_init"]), float(golden["am/bbox_thres"]))
    assert np.array_equal(lo.numpy(), golden["am/bbox_min"]) and np.array_equal(hi.numpy(), golden["am/bbox_max"])
    m = checkpoint.coarse_from_alphamask(VoxurfC, coarse_cfg("cpu", num_voxels=4000), rec, "cpu",
                                         float(golden["am/bbox_thres"]), float(golden["am/world_bound_scale"]), 0.2)
    assert isinstance(m, VoxurfC)
    assert np.array_equal(m.xyz_min.numpy(), golden["am/wide_min"]) and np.array_equal(m.xyz_max.numpy(), golden["am/wide_max"])
    assert np.array_equal(m.mask_xyz_min.numpy(), golden["am/xyz_min"]) and m.mask_alpha_init == float(golden["am/alpha_init"])
    assert np.array_equal(m.mask_cache.density.numpy(), golden["mc/pooled"])
    assert m.near == rec["near"] and m.far == rec["far"] and m.s_val == 0.2
    assert tuple(m.nonempty_mask.shape[2:]) == tuple(m.sdf.grid.shape[2:]) and bool(m.nonempty_mask.any())
    # without widening the box is the golden's own
    m1 = checkpoint.coarse_from_alphamask(VoxurfC, coarse_cfg("cpu", num_voxels=4000), rec, "cpu",
                                          float(golden["am/bbox_thres"]), 1.0, 0.2)
    assert np.array_equal(m1.xyz_min.numpy(), golden["am/bbox_min"]) and np.array_equal(m1.xyz_max.numpy(), golden["am/bbox_max"])
    rec["params"]["density"] = torch.full_like(rec["params"]["density"], -10.0)
    with pytest.raises(ValueError):
        checkpoint.coarse_from_alphamask(VoxurfC, coarse_cfg("cpu", num_voxels=4000), rec, "cpu", 1e-3, 1.05, 0.2)
