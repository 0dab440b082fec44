"""The coarse feature restatement (coarse_feat_ref64.py) checked on the CPU: the explicit adjoint against float64 autograd of the
restatement's own forward; a plain binary32 torch emulation inside the GPU test's bound and bit expectations on every input set of the
GPU test; a fixed list of mutants of that emulation each outside the bound (or against a bit expectation) on a small input set of
every operation it applies to; and the census of the classes the cases claim.  No GPU."""
import pytest
import torch

import coarse_feat_ref64 as R

F64 = torch.float64


@pytest.mark.parametrize("name", [c for c in R.CASES if not R.is_big(c)])
def test_backward_is_autograd_of_the_forward(name):
    inp = R.case(name)
    P = R.positions(inp)
    grids = {k: R._cl(inp[k].double()).clone().requires_grad_(True) for k in ("off_color", "emo_color", "grad_grid")}
    r = R.fwd_q(inp, P, grids)
    dO, dE = R._untile(inp["dX_off"]).double(), R._untile(inp["dX_emo"]).double()
    live, on = P.live[:, None].double(), (P.on & P.live)[:, None].double()
    loss = (dO[:, :12] * r.off.v * live).sum() + (dE[:, :12] * r.emo.v * on).sum() + ((dO[:, 24:27] * live + dE[:, 24:27] * on) * r.normal.v).sum()
    want = torch.autograd.grad(loss, [grids["off_color"], grids["emo_color"], grids["grad_grid"]], allow_unused=True)
    vals = R.bwd_values(inp, P, R.Q(r.normal.v.detach()), R.Q(r.nrm.v.detach()))
    W = r.W
    for w, v, (out, _, C) in zip(want, vals, R.BWD_OUT):
        contrib = R.Q(v.v[:, None, None, :], v.E[:, None, None, :]) * R.Q(W.v[..., None], W.E[..., None])
        val, _, touched = R.scatter_cells(inp, P.G, contrib, torch.zeros(C, w.shape[1], dtype=F64), torch.zeros(1, dtype=torch.long))
        w = torch.zeros_like(val) if w is None else w
        scale = float(w.abs().max())
        if out == "g_emo_color" and inp["Ton"] == 0:
            assert scale == 0 and not bool(touched.any())
            continue
        assert scale > 0
        assert float((val - w).abs().max()) <= 1e-11 * scale, (out, float((val - w).abs().max()) / scale)
        assert bool((w[~touched] == 0).all())


@pytest.mark.parametrize("op,case", R.all_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_binary32_emulation_is_inside_the_gpu_bound(op, case):
    inp = R.build(op, case)
    got = R.OPS[op][3](inp)
    ref, worst, fails = R.verify(op, inp, got, R.K_FAMILY[R.OPS[op][4]])
    assert not fails, fails
    assert ref.share == 0 and not ref.flips
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


CLASSES = {"1 tiles", "2 tiles", "9 tiles", "second trip", "grid 5x4x3", "grid 16x16x16", "tiles_on = 0", "tiles_on = 1", "tiles_on = tiles_all",
           "tiles_on inside", "emo_color, dX_emo and g_emo_color NULL", "padding lanes at the end of the on block",
           "padding lanes at the end of the off block", "a whole padding tile", "|g| = 0", "|g| below eps", "|g| of order 1",
           "point on a grid node", "boundary cell with corners off the grid", "point with no corner on the grid", "zero entries in dX",
           "non-zero initial gradient buffers"}


def test_the_cases_reach_every_class():
    u = set().union(*[R.case(c)["census"] for c in R.CASES])
    assert CLASSES <= u, CLASSES - u
    assert [R.is_big(c) for c in R.CASES].count(True) == 1 and R.CASES[R.BIG]["T"] == 2048 * 256 // 32 + 3
    # every tiles_on class on both grids' small cases, and a whole padding tile inside the on block and inside the off block
    small = [c for n, c in R.CASES.items() if not R.is_big(n)]
    assert {(c["grid"], c["Ton"] == 0) for c in small} >= {("5x4x3", True), ("5x4x3", False), ("16x16x16", True), ("16x16x16", False)}
    assert any(c["pad_tile"] is not None and c["pad_tile"] < c["Ton"] for c in small)
    assert any(c["pad_tile"] is not None and c["pad_tile"] >= c["Ton"] for c in small)
