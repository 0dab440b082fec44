"""The MLP restatement (mlp_ref64.py) checked on the CPU: the mask decoder and encoder are inverses and follow the documented bit
order; the forward restatement is torch's float64 `linear` chain on the reference's column order; a binary32 emulation of every entry
point (plain torch float32 `linear`; for the split engine two fp16 planes and three products accumulated in fp32) passes the GPU
test's checks on every input set of the GPU test (the bound is not too tight, the inputs are admissible); and a fixed list of
mutants of that emulation each fail them on at least one small input set of every operation they are listed for (the checks have
teeth).  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import mlp_ref64 as R

F64 = torch.float64
WORST, CAUGHT = {}, {}


# ---- the helpers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hid", [128, 192])
def test_mask_decoder_and_encoder_are_inverses(hid):
    g = torch.Generator().manual_seed(hid)
    M = torch.randint(-2 ** 31, 2 ** 31 - 1, (3, hid // 64, 64), generator=g, dtype=torch.int64).to(torch.int32)
    m = R.mask_decode(M, hid)
    assert m.shape == (3, hid, 32) and torch.equal(R.mask_encode(m), M)
    m2 = torch.rand(2, hid, 32, generator=g) < 0.3
    assert torch.equal(R.mask_decode(R.mask_encode(m2), hid), m2)


def test_mask_bit_order_is_the_documented_one():
    """bit b of word wd in lane s + 32 h is feature 32 (2 wd + (b >> 4)) + acc_row(b & 15, h) of sample s"""
    for wd, h, s, b in [(0, 0, 0, 0), (1, 1, 5, 17), (2, 0, 31, 31), (0, 1, 9, 4), (2, 1, 0, 16)]:
        M = torch.zeros(1, 3, 64, dtype=torch.int64)
        M[0, wd, s + 32 * h] = 1 << b
        M = torch.where(M >= 2 ** 31, M - 2 ** 32, M).to(torch.int32)
        m = R.mask_decode(M, 192)
        r = b & 15
        f = 32 * (2 * wd + (b >> 4)) + (r & 3) + 8 * (r >> 2) + 4 * h
        assert int(m.sum()) == 1 and bool(m[0, f, s]), (wd, h, s, b, torch.nonzero(m))
    # the lane halves of one register are four features apart
    assert R.acc_row(5, 1) - R.acc_row(5, 0) == 4 and sorted(R.acc_row(r, h) for r in range(16) for h in range(2)) == list(range(32))


@pytest.mark.parametrize("kind", list(R.NETS))
def test_forward_restatement_is_the_float64_linear_chain(kind):
    net = R.NETS[kind]
    g = torch.Generator().manual_seed(kind)
    Ws, Bs = R.make_net(kind, g)
    crow = net.crows[-1]
    X = R.make_X(kind, 2, g)
    x = R.x_ref(net, X, crow).double()
    # the reference's column order, written out: column c comes from the one row that maps to it
    for r in range(net.xrows):
        if net.colmap[r] >= 0:
            src = r + crow if r < net.cw else r
            assert torch.equal(x[:, net.colmap[r]], R.rm(X[:, src:src + 1]).double()[:, 0])
    pres, hs, (z, Ez) = R.fwd_chain(net, Ws, Bs, x, "q")
    h = x
    for l in range(net.nl):
        h = F.linear(h, Ws[l].double(), Bs[l].double())
        if l < net.nl - 1:
            assert torch.allclose(pres[l][0], h, rtol=1e-13, atol=1e-13)
            h = torch.relu(h)
    assert torch.allclose(z, h, rtol=1e-13, atol=1e-13) and bool((Ez > 0).all())


@pytest.mark.parametrize("kind", list(R.NETS))
def test_gradient_restatements_are_autograd_of_the_forward(kind):
    net = R.NETS[kind]
    g = torch.Generator().manual_seed(10 + kind)
    Ws, Bs = R.make_net(kind, g, plant=False)
    W64 = [w.double().requires_grad_(True) for w in Ws]
    B64 = [b.double().requires_grad_(True) for b in Bs]
    X = R.make_X(kind, 2, g)
    x = R.x_ref(net, X, 0).double().requires_grad_(True)
    h, hs = x, []
    for l in range(net.nl):
        h = F.linear(h, W64[l], B64[l])
        if l < net.nl - 1:
            h = torch.relu(h)
            hs.append(h)
    dz = torch.zeros(2, net.zrows, 32)
    dz[:, :net.out_dim] = torch.randn(2, net.out_dim, 32, generator=g)
    grads = torch.autograd.grad((h * R.rm(dz)[:, :net.out_dim].double()).sum(), [x] + W64 + B64)
    masks = [hh.detach() > 0 for hh in hs]
    dZ, (dx, _) = R.dgrad_chain(net, Ws, R.rm(dz), masks, "q")
    assert torch.allclose(dx, grads[0], rtol=1e-12, atol=1e-14)
    job = dict(kind=kind, crow=0, t0=0, t1=2, X=X, H=[R.tm(hh.detach().float(), 2) for hh in hs], dZ=[R.tm(d[0].float(), 2) for d in dZ], dz=dz)
    A, Bm = R._wg_pairs(job)
    for l in range(net.nl):
        assert torch.allclose(A[l].double().t() @ Bm[l].double(), grads[1 + l], rtol=1e-5, atol=1e-6)      # (operands rounded to binary32)
        assert torch.allclose(A[l].double().sum(0), grads[1 + net.nl + l], rtol=1e-5, atol=1e-6)


def test_gain_bound_and_amax_formula():
    g = torch.Generator().manual_seed(3)
    Ws, _ = R.make_net(R.RADIANCE, g)
    cs = [float(w.double().abs().sum(0).max()) for w in Ws]
    assert R.gain_bound(Ws) == max(1.0, cs[3], cs[3] * cs[2], cs[3] * cs[2] * cs[1])
    assert R.amax_formula32(0.5, 8.0) == 0.5 and R.amax_formula32(0.5, 64.0) == 2.0


def test_tone_cases_record_the_first_seed_without_a_decision_in_doubt():
    for name, cfg in R.TONE_CASES.items():
        if not cfg.get("big"):
            assert R.tone_first_seed(name) == cfg["seed"] <= cfg["seed0"] + R.TONE_MAX_REDRAWS, name


# ---- the emulation inside the bound, on every input set of the GPU test -----------------------------------------------
@pytest.mark.parametrize("op,case", R.all_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_binary32_emulation_passes_the_gpu_checks(op, case):
    inp = R.build(op, case)
    fam = R.OPS[op][4]
    ref, worst, fails = R.verify(op, inp, R.OPS[op][3](inp), R.K_FAMILY[fam])
    WORST[fam] = max(WORST.get(fam, 0.0), worst)
    print(f"\n[{op} {case}] worst |emulation - ref| / (U absref) = {worst:.3g}; {ref.note}")
    assert not fails, fails


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutant_of_the_emulation_fails_the_gpu_checks(mutant):
    caught = {}
    for op in R.MUTANTS[mutant]:
        for case in R.OPS[op][1]:
            if R.is_big(op, case):
                continue                                             # (small cases only)
            inp = R.build(op, case)
            if inp.get("einval") or inp.get("ecap"):
                continue
            _, _, fails = R.verify(op, inp, R.OPS[op][3](inp, mutant), R.K_FAMILY[R.OPS[op][4]])
            if fails:
                caught.setdefault(op, []).append(case)
    CAUGHT[mutant] = caught
    print(f"\n[{mutant}] caught by", caught)
    assert set(caught) == set(R.MUTANTS[mutant]), f"mutant `{mutant}` survives on {set(R.MUTANTS[mutant]) - set(caught)}"


def test_the_report():
    """the emulation's worst ratio per family (what seeded K_FAMILY before the GPU run) and the cases that catch each mutant"""
    print("\nworst ratio of the emulation per family:", {k: round(v, 4) for k, v in sorted(WORST.items())})
    for m, c in CAUGHT.items():
        print(f"{m}: " + "; ".join(f"{op}: {', '.join(cs)}" for op, cs in c.items()))
    assert set(WORST) <= set(R.K_FAMILY)
