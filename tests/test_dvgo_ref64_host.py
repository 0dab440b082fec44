"""The DVGO restatement (dvgo_ref64.py) checked on the CPU: the explicit adjoint against float64 autograd of the restatement's own
forward; the binary32 emulation (runs, wave scans in the kernel's order, the per-lane cell accumulator) inside the GPU test's bound
and bit expectations on every input set of the GPU test; a fixed list of mutants of that emulation each outside the bound (or
against a bit expectation) on a small input set of every operation it applies to; the census of the classes the cases claim; and
the share of banded decisions of the restatement alone.  No GPU."""
import pytest
import torch

import dvgo_ref64 as R

F64 = torch.float64


def _ids(v):
    return str(v).replace(" ", "")


# ---- adjoint = autograd of the forward --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice_S11_n10_ramp", "lattice_S65_n12_opaque", "g543_S129_n4_far", "g543_S128_n12", "g162_S129_n12",
                                  "lattice_S2_n3", "lattice_S63_n4", "lattice_S64_n5", "g543_S127_n5"])
def test_backward_is_autograd_of_the_forward(name):
    inp = R.case_train(name)
    G = R.sampling(inp)
    grids = {k: v.clone().requires_grad_(True) for k, v in R._grids64(inp).items()}
    r = R.fwd_q(inp, G, grids=grids)
    N, S = G.masked.shape
    loss = torch.zeros((), dtype=F64)
    for key, t in (("g_alphainv_cum", r.T.v), ("g_weights", r.w.v), ("g_raw_rgb", r.raw.v), ("g_rgb", r.rgb.v)):
        if inp[key] is not None:
            loss = loss + (inp[key].double() * t).sum()
    assert loss.requires_grad
    want = torch.autograd.grad(loss, [grids["density"], grids["off_color"], grids["emo_color"]], allow_unused=True)
    want = torch.cat([torch.zeros_like(g) if w is None else w for w, g in zip(want, grids.values())], 0)
    q = lambda t: R.Q(t.detach())
    vals, W = R.bwd_values(inp, G, q(r.a.v), q(r.T.v), q(r.raw.v), r.clamped)
    contrib = vals[..., None, :] * R.Q(W.v[..., None], W.E[..., None])
    val, absref, touched = R.scatter_cells(inp, G, contrib, torch.zeros_like(want), torch.arange(S) // R.run_len(S)[0])
    scale = float(want.abs().max())
    assert scale > 0
    assert float((val - want).abs().max()) <= 1e-11 * scale, float((val - want).abs().max()) / scale
    assert bool((want[~touched] == 0).all())


# ---- the emulation inside the bound, on every input set of the GPU test -----------------------------------------------
@pytest.mark.parametrize("op,case", R.all_cases(), ids=_ids)
def test_binary32_emulation_is_inside_the_gpu_bound(op, case):
    inp = R.build(op, case)
    got = R.OPS[op][3](inp)
    ref, worst, fails = R.verify(op, inp, got, R.K_FAMILY[R.OPS[op][4]])
    assert not fails, fails
    assert ref.share <= R.FLIP_CAP
    assert inp["claims"] <= inp["census"], inp["claims"] - inp["census"]


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutant_of_the_emulation_breaks_the_bound(mutant):
    killed = set()
    for op in R.MUTANTS[mutant]:
        for case in R.OPS[op][1]:
            if R.is_big(case) or op in killed:
                continue                                             # (small cases only)
            inp = R.build(op, case)
            _, _, fails = R.verify(op, inp, R.OPS[op][3](inp, mutant), R.K_FAMILY[R.OPS[op][4]])
            if fails:
                killed.add(op)
    assert killed == set(R.MUTANTS[mutant]), f"mutant `{mutant}` survives on {set(R.MUTANTS[mutant]) - killed}"


@pytest.mark.parametrize("case", ["lattice_S65_n12_opaque", "g162_S129_n12", "g543_S200_n13"])
def test_the_owner_of_the_last_transmittance_is_pinned_where_tail_lanes_are_empty(case):
    """S = 65, 129, 200: the owner (S - 1) / K sits in the middle of the wave; a T_S taken from the lane (S - 1) mod 64 leaves the bound"""
    for op in ("dvgo_fwd", "dvgo_eval"):
        inp = R.build(op, case)
        assert "owner of the last sample in the middle of the wave" in inp["census"]
        _, _, fails = R.verify(op, inp, R.OPS[op][3](inp, "last_transmittance_owner_ignores_run_length"), R.K_FAMILY["dvgo_fwd"])
        assert fails, (op, case)


# ---- the restatement's own banded decisions ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c for c in R.TRAIN_CASES if not R.is_big(c)])
def test_the_restatement_alone_meets_the_flip_cap(name):
    """the share of samples whose float64 exponential lies inside the band of 2^-25 (the only ones a kernel may decide otherwise)"""
    inp = R.case_train(name)
    G = R.sampling(inp)
    r = R.fwd_q(inp, G)
    band = ((r.e.v - R.E_CLAMP).abs() < R.DEC_K * R.U * r.e.E) & ~G.masked
    assert int(band.sum()) / band.numel() <= R.FLIP_CAP, int(band.sum())


def test_the_view_count_band_meets_the_flip_cap():
    for name in R.COUNT_CASES:
        inp = R.case_count(name)
        val, absref, _ = R.count_parts(inp)
        band = ((val - 1.0).abs() < R.DEC_K * R.U * absref)
        assert int(band.sum()) / band.numel() <= R.FLIP_CAP, (name, int(band.sum()))
    # the lattice-aligned set-up puts sums of exactly 1 on voxels: they are bit checks (absref 0), not banded
    val, absref, _ = R.count_parts(R.case_count("lattice_S9_n10"))
    assert bool(((val == 1.0) & (absref == 0)).any())


# ---- the census -------------------------------------------------------------------------------------------------------
S_CLASSES = {f"S = {s}" for s in (1, 2, 63, 64, 65, 127, 128, 129, 200)} | {f"K = {k}" for k in (1, 2, 3, 4)} | {
    "ragged last run", "empty tail lanes", "owner of the last sample in the middle of the wave", "lane 63 owns a sample", "second trip",
    "1 rays", "3 rays", "4 rays", "5 rays", "more than 5 rays"}
GRID_CLASSES = {f"grid {g}" for g in R.GRIDS} | {"axis of length 1"} | {f"step {s} voxels" for s in (0.1, 0.5, 1.0, 2.5, 7.0)}
RAY_CLASSES = {"exact-zero direction component", "origin inside the box", "ray misses the box", "sample on a node",
               "cell of base -1 with corners on the grid", "cell of base dims - 1 with corners on the grid", "no move", "far move",
               "single-axis move +1", "single-axis move -1", "three-axis move +1", "three-axis move -1", "move with mixed signs (+1, -1, 0)",
               "three or more samples of a run in one cell"}
INPUT_CLASSES = {"jitter NULL", "jitter zero", "jitter 0.999", "jitter random", "em_modes NULL, em_all 0", "em_modes NULL, em_all 1",
                 "em_modes mixed, with the value 2"}
DENSITY_CLASSES = {f"density {k}" for k in ("smooth", "empty", "opaque", "mixed", "ramp")} | {
    "alpha exactly 0 inside the box", "alpha exactly 1", "subnormal T", "T exactly 0", "alpha on both sides of the 2^-25 threshold"}
UP_CLASSES = {f"upstream {k}" for k in R.UP_KINDS} | {"zeros planted in the upstream gradients"}


def union(op):
    return set().union(*[R.build(op, c)["census"] for c in R.OPS[op][1]])


def test_the_cases_reach_every_class():
    for op in ("dvgo_fwd", "dvgo_bwd"):
        u = union(op)
        for cls in (S_CLASSES, GRID_CLASSES, RAY_CLASSES, INPUT_CLASSES, DENSITY_CLASSES, UP_CLASSES, {"leaves the box inside a run"}):
            assert cls <= u, (op, cls - u)
    u = union("dvgo_eval")
    for cls in (S_CLASSES - {"second trip"}, GRID_CLASSES, RAY_CLASSES, DENSITY_CLASSES):
        assert cls <= u, ("dvgo_eval", cls - u)
    u = union("dvgo_count")
    want = GRID_CLASSES | (RAY_CLASSES - {"origin inside the box"}) | {"second trip", "1 rays", "3 rays", "5 rays", "more than 5 rays",
                                                                       "jitter NULL", "jitter random", "jitter 0.999", "sum starts at 0",
                                                                       "sum starts non-zero"}
    assert want <= u, want - u
    assert sum(R.is_big(c) for _, c in R.all_cases()) == 3
    assert R.case_train(R.BIG_TRAIN)["rep"].numel() == 65541 and R.case_count(R.BIG_COUNT)["rep"].numel() > 256 * 16384


def test_the_saturation_ramp_straddles_the_threshold():
    inp = R.case_train("lattice_S11_n10_ramp")
    G = R.sampling(inp)
    r = R.fwd_q(inp, G)
    t = -torch.log(r.e.v[0, :9])
    assert float(t.min()) < 16.9 and float(t.max()) > 17.7 and bool(r.clamp64[0, :3].all()) and not bool(r.clamp64[0, 5:9].any())
