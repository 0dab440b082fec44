"""The shading / compositing / loss restatement (shade_ref64.py) checked on the CPU: every backward against float64 autograd of
the restatement's own forward; a plain binary32 torch emulation of every entry point inside the GPU test's bound on every
input set of the GPU test (the bound is not too tight, the inputs are admissible, the decision flips stay under their cap);
and a fixed list of mutants of that emulation each outside the bound on at least one of those input sets (the bound has
teeth).  No GPU."""
import pytest
import torch

import shade_ref64 as R

F64 = torch.float64
REL = 1e-12


def _close(a, b, what):
    a, b = a.double(), b.double()
    assert float((a - b).abs().max()) <= REL * max(float(b.abs().max()), 1e-300), what


def _smooth(name):
    """a tile case with smooth pre-activations (no value on a threshold) in float64"""
    d = dict(R.tile_base(name))
    g = torch.Generator().manual_seed(1)
    for k in ("z_off", "z_emo", "zt"):
        d[k] = (torch.randn(d[k].shape, generator=g, dtype=F64) * 3)
    for k in ("rec_w", "g_srgb", "g_lin", "g_wbg", "dXt"):
        d[k] = d[k].double() / d["gscale"] if k != "rec_w" else d[k].double()
    return d


def _live(d):
    return (d["rec_ray"] >= 0), d["rec_ray"].clamp_min(0).long()


@pytest.mark.parametrize("name", ["odd", "even"])
@pytest.mark.parametrize("lts", [False, True])
def test_tone_in_backward_is_autograd_of_the_forward(name, lts):
    d = _smooth(name)
    live, ray = _live(d)
    T, t_on = d["tiles_all"], d["tiles_on"]
    zo, ze = d["z_off"].clone().requires_grad_(True), d["z_emo"].clone().requires_grad_(True)
    lin, _ = R.lin64(zo, ze, t_on, detach_off=not lts)
    X = R.xt64(lin)
    m = live.reshape(T, 1, 32).double()
    w = (d["rec_w"] * live).reshape(T, 1, 32)
    gl = d["g_lin"][ray].reshape(T, 32, 3).permute(0, 2, 1)
    L = (d["dXt"][:, :33] * m * X).sum() + (w * gl * lin).sum()
    go, ge = torch.autograd.grad(L, (zo, ze))
    Xt = torch.zeros(T, R.XT_ROWS, 32, dtype=F64)
    Xt[:, :33] = X.detach()
    d["Xt"] = Xt
    if lts:
        r = R.ref_lts_tone_in_bwd(d).out
        _close(r["dz_off"][0][:, :3], go[:, :3], "dz_off")
        _close(r["dz_emo"][0][:t_on, :3], ge[:t_on, :3], "dz_emo")
    else:
        r = R.ref_tone_in_bwd(d).out["dz"][0]
        _close(r[:t_on, :3], ge[:t_on, :3], "dz (on-tiles: emo)")
        _close(r[t_on:, :3], go[t_on:, :3], "dz (off-tiles: off)")
        assert float(go[:t_on].abs().max()) == 0.0               # the detach


@pytest.mark.parametrize("name", ["odd", "even"])
def test_composite_backward_is_autograd_of_the_forward(name):
    d = _smooth(name)
    live, ray = _live(d)
    zt, w = d["zt"].clone().requires_grad_(True), d["rec_w"].clone().requires_grad_(True)
    d["lin"] = d["lin"].double()
    col = torch.sigmoid(zt[:, :3])
    cs = torch.stack([R.ch(col, c) for c in range(3)], 1)
    ls = torch.stack([R.ch(d["lin"], c) for c in range(3)], 1)
    n = d["n_rays"]
    srgb = torch.zeros(n, 3, dtype=F64).index_add(0, ray[live], (w[:, None] * cs)[live])
    linm = torch.zeros(n, 3, dtype=F64).index_add(0, ray[live], (w[:, None] * ls)[live])
    fw = R.ref_composite_fwd(dict(d, zt=zt.detach(), rec_w=w.detach(), srgb0=torch.zeros(n, 3), lin0=torch.zeros(n, 3))).out
    _close(fw["srgb_marched"][0], srgb.detach(), "srgb_marched")
    _close(fw["lin_marched"][0], linm.detach(), "lin_marched")
    gz, gw = torch.autograd.grad((d["g_srgb"] * srgb).sum() + (d["g_lin"] * linm).sum(), (zt, w))
    rgb = torch.zeros_like(d["zt"])
    rgb[:, :3] = col.detach()
    r = R.ref_composite_bwd(dict(d, rgb=rgb)).out
    _close(r["dzt"][0][:, :3], gz[:, :3], "dzt")
    _close(r["dweight"][0], gw, "dweight")


@pytest.mark.parametrize("name", ["odd", "even"])
def test_composite3_and_coarse_backward_are_autograd_of_the_forward(name):
    d = _smooth(name)
    live, ray = _live(d)
    n, T, t_on = d["n_rays"], d["tiles_all"], d["tiles_on"]
    c3 = R.case_composite3(name)
    v, w = c3["v"].double().requires_grad_(True), d["rec_w"].clone().requires_grad_(True)
    vs = torch.stack([R.ch(v, c) for c in range(3)], 1)
    out = torch.zeros(n, 3, dtype=F64).index_add(0, ray[live], (w[:, None] * vs)[live])
    gv, gw = torch.autograd.grad((d["g_srgb"] * out).sum(), (v, w))
    r = R.ref_composite3_bwd(dict(c3, v=v.detach(), rec_w=w.detach(), g=d["g_srgb"], accumulate=0)).out
    _close(r["dv"][0][:, :3], gv[:, :3], "dv")
    _close(r["dweight"][0], gw, "dweight")
    # coarse: srgb = sum w rgb, white_bg = 1 - sum w
    zo, ze = d["z_off"].clone().requires_grad_(True), d["z_emo"].clone().requires_grad_(True)
    w = d["rec_w"].clone().requires_grad_(True)
    rgb, _ = R.coarse_rgb64(dict(d, z_off=zo, z_emo=ze))
    cs = torch.stack([R.ch(rgb, c) for c in range(3)], 1)
    srgb = torch.zeros(n, 3, dtype=F64).index_add(0, ray[live], (w[:, None] * cs)[live])
    wbg = 1 - torch.zeros(n, dtype=F64).index_add(0, ray[live], w[live])
    go, ge, gw = torch.autograd.grad((d["g_srgb"] * srgb).sum() + (d["g_wbg"] * wbg).sum(), (zo, ze, w))
    rgb4 = torch.zeros(T, 4, 32, dtype=F64)
    rgb4[:, :3] = rgb.detach()
    r = R.ref_coarse_shade_bwd(dict(d, rgb=rgb4)).out
    _close(r["dz_off"][0][:, :3], go[:, :3], "dz_off")
    _close(r["dz_emo"][0][:t_on, :3], ge[:t_on, :3], "dz_emo")
    _close(r["dweight"][0], gw, "dweight")


@pytest.mark.parametrize("white_bg,scale,last", [(1.0, 0.25, "inside"), (0.0, 1.0, "inside"), (1.0, 1.0, "below")])
def test_loss_gradients_are_autograd_of_the_value(white_bg, scale, last):
    d = R._loss_inputs(97, white_bg, scale, last, seed=3)
    leaves = {k: d[k].double().requires_grad_(True) for k in ("srgb_m", "lin_m", "last")}
    r = R.ref_loss(dict(d, **leaves))
    gs, gl, ga = torch.autograd.grad(r.loss_t, tuple(leaves.values()))
    _close(r.out["g_srgb"][0], gs, "g_srgb")
    _close(r.out["g_lin"][0], gl, "g_lin")
    _close(r.out["g_last"][0], ga, "g_last")


@pytest.mark.parametrize("act", [0, 1])
def test_act_and_pair_gradients_are_autograd(act):
    g = torch.Generator().manual_seed(act)
    z = (torch.randn(3, 4, 32, generator=g, dtype=F64) * 4).requires_grad_(True)
    up = torch.randn(3, 4, 32, generator=g, dtype=F64)
    fwd = torch.nn.functional.softplus(z, threshold=20) if act == 0 else torch.sigmoid(z)
    gz, = torch.autograd.grad((up * fwd).sum(), z)
    r = R.ref_act(dict(z=z.detach(), g=up, act=act, n_ch=4)).out
    _close(r["fwd"][0], fwd.detach(), "act forward")
    _close(r["bwd"][0], gz, "act backward")
    job = dict(R.pair_jobs()["mask_count" if act else "mse"], w_value=0.5, w_a=0.5, w_b=0.5)
    a, b = job["a"].double().requires_grad_(True), job["b"].double().requires_grad_(True)
    t = R.pair_term64(dict(job, a=a, b=b))
    ga, gb = torch.autograd.grad(t["value_t"], (a, b))
    _close(t["ga"][0], ga, "ga")
    _close(t["gb"][0], gb, "gb")


# ---- the emulation inside the bound, on every input set of the GPU test -----------------------------------------------
@pytest.mark.parametrize("op,case", R.all_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_binary32_emulation_is_inside_the_gpu_bound(op, case):
    inp = R.build(op, case)
    got = R.OPS[op][3](inp)
    ref, worst, fails = R.verify(op, inp, got, R.K_FAMILY[R.OPS[op][4]])
    assert not fails, fails
    assert ref.share <= R.FLIP_CAP, f"{ref.share:.3%} of the values exempted as decision flips"
    if "claims" in inp:
        assert inp["claims"] <= inp["census"], inp["claims"] - inp["census"]


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutant_of_the_emulation_breaks_the_bound(mutant):
    killed = []
    for op in R.MUTANTS[mutant]:
        for case in R.OPS[op][1]:
            if R.is_big(case):
                continue
            inp = R.build(op, case)
            try:
                _, _, fails = R.verify(op, inp, R.OPS[op][3](inp, mutant), R.K_FAMILY[R.OPS[op][4]])
            except AssertionError as e:                      # a forced decision off its boundary is a rejection too
                fails = [str(e)]
            if fails:
                killed.append((op, case))
    assert killed, f"mutant `{mutant}` passes the bound on every case of {R.MUTANTS[mutant]}"
    ops_hit = {op for op, _ in killed}
    assert ops_hit == set(R.MUTANTS[mutant]), f"mutant `{mutant}` survives on {set(R.MUTANTS[mutant]) - ops_hit}"
