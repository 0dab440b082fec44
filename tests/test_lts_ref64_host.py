"""The light-transport restatement (lts_ref64.py) checked on the CPU: every backward against float64 autograd of the restatement's
own forward; every forward against oracle/lts_path.py evaluated in float64 on smooth inputs; a plain binary32 torch emulation of
every entry point inside the GPU test's bound on every input set of the GPU test (the bound is not too tight, the inputs are
admissible, the decision flips stay under their cap); and a fixed list of mutants of that emulation each outside the bound on at
least one of those input sets (the bound has teeth).  No GPU."""
import math
from types import SimpleNamespace

import pytest
import torch

import lts_ref64 as R
from oracle import lts_path as lp

F64 = torch.float64
REL = 1e-12
EXACT = R.Consts(exact=True)


def _close(a, b, what):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, what
    assert float((a - b).abs().max()) <= REL * max(float(b.abs().max()), 1e-300), (what, float((a - b).abs().max()), float(b.abs().max()))


# ---- backward = autograd of the forward -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p255", "p257", "ray", "rayz"])
def test_expgrad_backward_is_autograd_of_the_forward(name):
    inp = dict(R.case_expgrad(name))
    grid = inp["sdf"].double().requires_grad_(True)
    fw = R.ref_expgrad_fwd(inp, sdf=grid)
    (gg,) = torch.autograd.grad((inp["g"].double() * fw.q.v).sum(), grid)
    bw = R.ref_expgrad_bwd(dict(inp, grad0=torch.zeros_like(inp["grad0"])))
    _close(bw.out["grad_sdf"][0].reshape(gg.shape), gg, "grad_sdf")
    assert float(gg.abs().max()) > 0.1


@pytest.mark.parametrize("name", ["p1r1j1", "p3r64j1", "p10r8j48", "p10r8j48_pdra", "p5r257j64_pdra", "p7r300j48"])
def test_combine_backward_is_autograd_of_the_forward(name):
    inp = dict(R.case_combine(name))
    keys = ("base", "rough", "metal", "off_m", "emo_m", "last2", "emission", "mus", "lambdas", "lobes")
    leaves = {k: inp[k].double().requires_grad_(True) for k in keys}
    oh, eh, _ = R._combine_fwd_any(inp, "64", leaves=leaves)
    L = (inp["g_off_hat"].double() * oh).sum() + (inp["g_emo_hat"].double() * eh).sum()
    gr = dict(zip(keys, torch.autograd.grad(L, tuple(leaves.values()), allow_unused=True)))
    zero = dict(inp, **{k: torch.zeros_like(inp[k]) for k in ("d_mus0", "d_lambdas0", "d_lobes0")})
    out = R.ref_lts_combine_bwd(zero).out
    for mine, k in (("d_base", "base"), ("d_rough", "rough"), ("d_metal", "metal"), ("d_off_m", "off_m"), ("d_emo_m", "emo_m"),
                    ("d_last2", "last2"), ("d_emission", "emission"), ("d_mus", "mus"), ("d_lambdas", "lambdas"), ("d_lobes", "lobes")):
        want = gr[k] if gr[k] is not None else torch.zeros_like(leaves[k])
        _close(out[mine][0], want, mine)


# ---- forward = the oracle in float64 ----------------------------------------------------------------------------------
def test_expgrad_forward_is_the_oracle():
    g = torch.Generator().manual_seed(1)
    lo, hi = R.EG_LO.double(), R.EG_HI.double()
    grid = torch.randn(*R.EG_DIMS, generator=g, dtype=F64)
    pts = lo + (hi - lo) * torch.rand(200, 3, generator=g, dtype=F64)
    sdf, gr = lp.sdf_expgrad(SimpleNamespace(xyz_min=lo, xyz_max=hi), grid[None, None], pts)
    out = R.ref_expgrad_fwd(dict(pts=pts, lo=lo, hi=hi, dims=R.EG_DIMS, sdf=grid, zero_pad=0)).out["out"][0]
    _close(out[:, 0], sdf.detach(), "value")
    _close(out[:, 1:], gr.detach(), "gradient")


def test_dirs_forward_is_the_oracle():
    g = torch.Generator().manual_seed(2)
    nrm = torch.nn.functional.normalize(torch.randn(9, 3, generator=g, dtype=F64), dim=-1)
    raw = torch.randn(9, 17, 3, generator=g, dtype=F64)
    _close(R.ref_lts_dirs(dict(raw=raw, normal=nrm)).out["dirs"][0], lp.hemisphere_dirs(nrm, raw), "dirs")


def _smooth_combine(pdra):
    g = torch.Generator().manual_seed(3 + pdra)
    P, Rr, J = 6, 11, 5
    rn = lambda *s: torch.rand(*s, generator=g, dtype=F64)
    nz = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    unit = lambda t: torch.nn.functional.normalize(t, dim=-1)
    nrm = unit(nz(P, 3))
    return dict(P=P, R=Rr, J=J, pdra=pdra, base=rn(P, 3), rough=0.05 + 0.95 * rn(P), metal=rn(P), normal=nrm, view=unit(nz(P, 3)),
                dirs=lp.hemisphere_dirs(nrm, nz(P, Rr + 1, 3)), off_m=rn(P * Rr, 3) * 2, emo_m=rn(P * Rr, 3) * 2, last2=rn(P * Rr),
                mus=nz(J, 3) * 0.3, lambdas=10 + 20 * nz(J), lobes=nz(J, 3), emission=rn(P, 3),
                umask=(torch.arange(P) % 3 == 0).to(torch.uint8))


@pytest.mark.parametrize("pdra", [0, 1])
def test_combine_forward_is_the_oracle(pdra):
    d = _smooth_combine(pdra)
    P, Rr = d["P"], d["R"]
    rep = lambda t: t.repeat([2] + [1] * (t.dim() - 1))
    ex = lambda t: t.view(P, 1, -1).expand(P, Rr, t.shape[-1]).flatten(0, 1)
    d2, v_rand = d["dirs"][:, :-1].flatten(0, 1), -d["dirs"][:, -1]
    Rf = lp.disney_reflection(rep(ex(d["base"])), rep(ex(d["rough"][:, None])), rep(ex(d["metal"][:, None])), rep(ex(d["normal"])),
                              rep(d2), torch.cat([-ex(d["view"]), -ex(v_rand)], 0))
    Pm = {"envmap.mus": d["mus"], "envmap.lambdas": d["lambdas"][:, None], "envmap.lobes": d["lobes"]}
    env = lp.sg_envmap(Pm, d2)
    off_hat = (rep(d["off_m"] + env * d["last2"][:, None]) * Rf).view(-1, Rr, 3).mean(-2)
    reflect = (rep(d["emo_m"]) * Rf).view(-1, Rr, 3).mean(-2)
    um = rep(d["umask"].bool())
    emo_hat = torch.where(um[:, None], rep(d["emission"]) + reflect, reflect) if pdra else rep(d["emission"]) + reflect
    oh, eh, c = R._combine_fwd_any(d, "64", EXACT)
    _close(c["env"].reshape(-1, 3), env, "sg_envmap")
    _close(torch.cat([c["d"][0][0], c["d"][1][0]]).reshape(-1, 3), Rf, "disney_reflection")
    _close(oh, off_hat, "off_hat")
    _close(eh, emo_hat, "emo_hat")
    q = R.ref_lts_combine_fwd(d, EXACT).out                           # (the Q arithmetic carries the same values)
    _close(q["off_hat"][0], off_hat, "off_hat (Q)")


def test_emit_edit_is_the_oracle():
    g = torch.Generator().manual_seed(5)
    n = 60
    emit = torch.rand(n, 3, generator=g, dtype=F64) * 4 + 1e-3
    modes = torch.arange(n) % 5
    inten = torch.rand(n, generator=g, dtype=F64) * 3
    cols = torch.rand(n, 2, generator=g, dtype=F64)
    cols[:, 0] = torch.randint(0, 64, (n,), generator=g).double() / 64          # h 6 is a binary32 number: the replay is exact
    _close(R._emit_any(dict(emit=emit, modes=modes, inten=inten, colors=cols), "64"), lp.edit_emission(emit, modes, inten, cols), "emit")


def test_no_roughness_squares_onto_the_r2_threshold():
    """ro * ro, rounded, never equals 1e-7f: the neighbours of sqrt(1e-7) land one ulp below and two above"""
    e = torch.tensor(1e-7, dtype=torch.float32)
    r = torch.tensor(math.sqrt(1e-7), dtype=torch.float32)
    c = (r.view(torch.int32) + torch.arange(-64, 65, dtype=torch.int32)).view(torch.float32)
    sq = (c.double() ** 2).float()
    assert bool((sq[:-1] <= sq[1:]).all()) and bool((sq[0] < e) & (sq[-1] > e)) and not bool((sq == e).any())
    assert float((R._ro_above_threshold().double() ** 2).float()) == float(sq[sq > e].min())


# ---- the emulation inside the bound, on every input set of the GPU test -----------------------------------------------
@pytest.mark.parametrize("op,case", R.all_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_binary32_emulation_is_inside_the_gpu_bound(op, case):
    inp = R.build(op, case)
    got = R.OPS[op][3](inp)
    ref, worst, fails = R.verify(op, inp, got, R.K_FAMILY[R.OPS[op][4]])
    assert not fails, fails
    assert ref.share <= R.FLIP_CAP, f"{ref.share:.3%} of the values exempted as decision flips"
    assert inp["claims"] <= inp["census"], inp["claims"] - inp["census"]


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutant_of_the_emulation_breaks_the_bound(mutant):
    killed = []
    for op in R.MUTANTS[mutant]:
        for case in R.OPS[op][1]:
            if isinstance(case, str) and case.startswith("p5000"):
                continue                                             # (small cases only)
            inp = R.build(op, case)
            ref, _, fails = R.verify(op, inp, R.OPS[op][3](inp, mutant), R.K_FAMILY[R.OPS[op][4]])
            if fails or ref.share > R.FLIP_CAP:
                killed.append((op, case))
    ops_hit = {op for op, _ in killed}
    assert ops_hit == set(R.MUTANTS[mutant]), f"mutant `{mutant}` survives on {set(R.MUTANTS[mutant]) - ops_hit}"
