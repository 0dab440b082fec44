"""The dense-grid restatement (grid_ref64.py) checked on the CPU: the adjoints against float64 autograd of the restatement's own
forwards; a plain binary32 torch emulation of every entry point inside the GPU test's bound (and its bit expectations) on every
input set of the GPU test (the bound is not too tight, the inputs are admissible); a fixed list of mutants of that emulation each
outside the bound on at least one small input set of every operation it applies to (the bound has teeth); and the census of the
classes the cases claim.  No GPU."""
import pytest
import torch

import grid_ref64 as R

F64 = torch.float64
REL = 1e-12


def _close(a, b, what):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, what
    assert float((a - b).abs().max()) <= REL * max(float(b.abs().max()), 1e-300), (what, float((a - b).abs().max()))


# ---- adjoint = autograd of the forward --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1x1x7", "2x5x1", "3x3x3", "5x4x3", "9x7x6"])
def test_central_adjoint_is_autograd_of_the_forward(name):
    inp = R.case_central(name)
    s = inp["sdf"].double().requires_grad_(True)
    fw = torch.stack(R.central_any(s, inp["voxel"], "64"), -1)
    (gs,) = torch.autograd.grad((fw * inp["g"].double()).sum(), s)
    want = inp["gsdf0"].double() + gs
    _close(R._central_bwd_any(inp, "q").v, want, "gsdf")


@pytest.mark.parametrize("name", ["5x4x3_random", "9x7x6_full", "3x3x3_interior"])
def test_smooth_tv_backward_is_autograd_of_the_forward(name):
    """d loss / d sdf with the conv branch detached, from the error field of the forward's own restatement"""
    inp = dict(R.case_smooth(name))
    s = inp["sdf"].double().requires_grad_(True)
    g = torch.stack(R.central_any(s, inp["voxel"], "64"))
    sm = R.corr3(g.detach(), inp["w"].double(), 1) + inp["bias"]
    m = (inp["mask"] != 0)[None].expand_as(g)
    err = torch.where(m, sm - g, torch.zeros((), dtype=F64))
    inv = inp["weight"] / (3.0 * inp["mc"])
    (gs,) = torch.autograd.grad((err * err).sum() * inv * float(inp["grad_out"][0]), s)
    inp["work6"] = torch.cat([g.detach(), err.detach()])
    got = R._smooth_bwd_any(inp, True, "q").v
    want = inp["grad0"].double() + gs
    assert float((got - want).abs().max()) <= 1e-6 * float(gs.abs().max())        # (the coefficient is the entry's binary32 one)
    assert float(gs.abs().max()) > 0


def test_gauss_forward_is_the_oracle():
    from oracle.coarse_path import gaussian_kernel, smooth_grid
    inp = R.case_gauss("9x7x6_k5_gaussian")
    want = smooth_grid(inp["x"].double()[None, None], gaussian_kernel(5, 1.0).double())[0, 0]
    _close(R.corr3(inp["x"].double(), inp["w"].double(), 2), want, "gauss3d")


# ---- the emulation inside the bound, on every input set of the GPU test -----------------------------------------------
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


# ---- the census -------------------------------------------------------------------------------------------------------
STENCIL_CLASSES = {"corner", "edge", "face", "interior", "axis of length 1", "axis of length 2", "no interior cell", "second trip",
                   "every axis shorter than r = 3"}
TV_CLASSES = {f"{what} (axis {a}, {d:+d})" for what in ("difference exactly +-1", "difference beyond +-1", "equal neighbours")
              for a in (1, 2, 3) for d in (-1, 1)} | {"channel seam with a jump of 1e3", "wy != wz", "-0.0 and +0.0 gradients", "dense",
                                                     "sparse"}
MASK_CLASSES = {f"mask: {m}" for m in R.MASKS} | {"masked_cells = 0", "asymmetric weights, non-zero bias", "the product's symmetric kernel"}
ADAM_CLASSES = {"vector kernel", "scalar kernel", "scalar tail", "no whole float4", "second trip", "per_lr NULL", "per_lr zeros",
                "weight decay", "eps 0", "lr 0.0", "zero gradient", "gradient 1e-20 .. 1e18", "m = -g", "step 1", "step 2", "step 1000",
                "step 100000"} | {f"{w} offset by 4 bytes" for w in ("p", "g", "m", "v", "plr")}
LIVE_CLASSES = {"already live, zero gradient", "live byte 255", "dead brick", "gradient only in the ragged tail",
                "gradient only in the last lane", "-0.0 in a dead brick", "zero_grad 0", "zero_grad 1", "stats given", "stats NULL",
                "per_lr given", "per_lr NULL", "whole quads and a tail", "whole bricks and a ragged one in the tail", "second trip",
                "about 1 % of the bricks touched"}


def union(op):
    return set().union(*[R.build(op, c)["census"] for c in R.OPS[op][1]])


def test_the_cases_reach_every_class():
    for op in ("tv_add_grad", "smooth_tv_fwd", "gauss3d_bwd", "central_grad_bwd"):
        assert STENCIL_CLASSES <= union(op), (op, STENCIL_CLASSES - union(op))
    assert TV_CLASSES <= union("tv_add_grad"), TV_CLASSES - union("tv_add_grad")
    assert MASK_CLASSES <= union("smooth_tv_fwd"), MASK_CLASSES - union("smooth_tv_fwd")
    assert {f"k = {k}" for k in R.KS} | {"every axis shorter than r", "asymmetric weights"} <= union("gauss3d_fwd")
    assert ADAM_CLASSES <= union("adam_step"), ADAM_CLASSES - union("adam_step")
    assert LIVE_CLASSES <= union("adam_live"), LIVE_CLASSES - union("adam_live")
    assert {c["n"] for c in R.ADAM_CASES.values() if "n" in c} >= set(R.ADAM_NS) and R.ADAM_NS[-1] == 4 * 1048576 + 1203
    assert {c["n"] for c in R.LIVE_CASES.values()} == set(R.LIVE_NS) | {R.LIVE_BIG_N}
    # offset pointers with per_lr present and NULL
    offs = {(c.get("off"), "plr" in c and c["plr"] is None) for c in R.ADAM_CASES.values() if c.get("off")}
    assert offs >= {(w, False) for w in ("p", "g", "m", "v", "plr")} | {(w, True) for w in ("p", "g", "m", "v")}


def test_random_weights_have_no_symmetry():
    for name in ("9x7x6_k3", "9x7x6_k5", "9x7x6_k7", ):
        w = R.case_gauss(name)["w"]
        assert torch.unique(w).numel() == w.numel() and bool((w > 0).any()) and bool((w < 0).any())
    inp = R.case_smooth("9x7x6_full")
    assert torch.unique(inp["w"]).numel() == 27 and inp["bias"] != 0
