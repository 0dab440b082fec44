"""The bf16 MLP restatement (mlp_bf16_ref64.py) checked on the CPU: the float64 bf16 rounding agrees with torch's on every bf16
boundary case, the row-quad and X16 codecs follow the documented orders, an emulation of every entry point (torch bf16 rounding,
binary32 `linear`, the codecs in Python) passes the GPU test's checks on every small input set -- so the intervals are not too tight
and the two input conditions hold (ambiguous roundings <= 1/4, unchained decisions inside the band <= 1/100; `verify` reports either
as a failure) -- and a fixed list of mutants of that emulation each fail them on at least one small input set of every operation they
are listed for.  No GPU."""
import pytest
import torch

import mlp_bf16_ref64 as B
import mlp_ref64 as R

WORST, CAUGHT, NOTES = {}, {}, {}


def test_float64_bf16_rounding_is_round_to_nearest_even():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(20000, generator=g) * 10.0 ** (8.0 * torch.rand(20000, generator=g) - 4.0)
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 2 - 2.0 ** -9, 2 - 2.0 ** -8, -0.0, 0.0, -(1 + 2.0 ** -8), 3e-30, 7e30])
    x = torch.cat([x, ties])
    assert torch.equal(B.r16d(x.double()), B.r16(x).double())
    assert B.r16(ties[:4]).tolist() == [1.0, 1 + 2.0 ** -6, 2.0, 2.0]                 # even neighbour below, odd below, the next binade, a tie into it
    assert B.t16(ties[:4]).tolist() == [1.0, 1 + 2.0 ** -7, 2 - 2.0 ** -7, 2 - 2.0 ** -7]
    # a float64 just above / below a tie does not round as the tie does
    t = torch.tensor([1 + 2.0 ** -8], dtype=torch.float64)
    assert B.r16d(t + 2.0 ** -40).item() == 1 + 2.0 ** -7 and B.r16d(t - 2.0 ** -40).item() == 1.0
    # the interval of a computed value: one point away from a boundary, two bf16 neighbours across one
    mid, Eop, lo, hi = B.round_op(torch.tensor([1.001, 1 + 2.0 ** -8], dtype=torch.float64), torch.tensor([1.0, 1.0], dtype=torch.float64), 1.0)
    assert lo[0] == hi[0] == mid[0] and Eop[0] == 0 and (lo[1], hi[1]) == (1.0, 1 + 2.0 ** -7) and Eop[1] == 2.0 ** -7 / R.U


def test_row_quad_codec_is_the_documented_order():
    t = torch.arange(2 * 8 * 32, dtype=torch.float32).reshape(2, 8, 32)                   # (integers below 512: exact in bf16 up to 256 ...)
    t = t % 251
    b = B.rq_encode(t)
    assert b.shape == (2, 2, 32, 4) and b.dtype == torch.int16 and torch.equal(B.rq_decode(b), t)
    for tile, row, s in [(0, 0, 0), (1, 5, 1), (0, 7, 2), (1, 2, 9), (0, 4, 31), (1, 3, 16)]:
        slot = 8 * ((s >> 1) & 3) + 2 * (s >> 3) + (s & 1)
        assert b.view(torch.bfloat16)[tile, row // 4, slot, row % 4].item() == t[tile, row, s].item()
    assert sorted(B.SLOT.tolist()) == list(range(32))


def test_mask_bit_order_is_the_bf16_engines():
    """bit 8 (it & 1) + (r >> 1) + 16 (r & 1) of word it / 2 in lane s + 32 h is feature 32 it + acc_row(r, h) of sample s"""
    for it, r, h, s in [(0, 0, 0, 0), (1, 1, 1, 5), (5, 15, 0, 31), (2, 6, 1, 9), (3, 9, 1, 0)]:
        M = torch.zeros(1, 3, 64, dtype=torch.int64)
        M[0, it // 2, s + 32 * h] = 1 << (8 * (it & 1) + (r >> 1) + 16 * (r & 1))
        M = torch.where(M >= 2 ** 31, M - 2 ** 32, M).to(torch.int32)
        m = B.mask_decode(M, 192)
        assert int(m.sum()) == 1 and bool(m[0, 32 * it + R.acc_row(r, h), s]), (it, r, h, s, torch.nonzero(m))
    g = torch.Generator().manual_seed(3)
    M = torch.randint(-2 ** 31, 2 ** 31 - 1, (3, 2, 64), generator=g, dtype=torch.int64).to(torch.int32)
    assert torch.equal(B.mask_encode(B.mask_decode(M, 128)), M) and sorted(B.MASK_BIT16) == list(range(32))


def test_x16_tile_is_26_quads_with_the_second_colour_group_behind():
    X = R.make_X(R.RADIANCE, 2, torch.Generator().manual_seed(0))
    x16 = B.x16_tile(X)
    assert x16.shape == (2, 26, 32, 4)
    rows = B.rq_decode(x16)
    assert torch.equal(rows[:, :96], B.r16(X[:, :96])) and torch.equal(rows[:, 96:102], B.r16(X[:, 88:94])) and torch.equal(rows[:, 102:], B.r16(X[:, 6:8]))
    net = R.NETS[R.RADIANCE]
    for crow in (0, 88):
        assert torch.equal(R.x_ref(net, B.x16_rows(x16, crow), 0), B.r16(R.x_ref(net, X, crow)))


def test_tone_cases_record_the_first_seed_without_a_decision_in_doubt():
    for name, cfg in B.TONE_CASES.items():
        if not cfg.get("big"):
            assert B.tone_first_seed(name) == cfg["seed"] <= cfg["seed0"] + R.TONE_MAX_REDRAWS, name


def test_every_case_carries_the_planted_rounding_cases():
    want = [1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 2 - 2.0 ** -9]
    for inp, t in ((B.case_fwd("rad_t1"), B.case_fwd("rad_t1")["X"][0, 24]), (B.case_dgrad("tone_t1"), B.case_dgrad("tone_t1")["dz"][0, 0, 8:] * 64),
                   (B.case_fwd("brdf_t1"), B.case_fwd("brdf_t1")["nets"][0][0][1][7] * 8), (B.case_tone("t1"), B.case_tone("t1")["Xt"][0, 8] * 2)):
        assert t[:3].tolist() == want and t[3].item() == 0 and bool(torch.signbit(t[3])), inp["name"]


# ---- the emulation inside the checks, on every small input set of the GPU test -------------------------------------------
@pytest.mark.parametrize("op,case", [c for c in B.all_cases() if not B.is_big(*c)], ids=lambda v: str(v).replace(" ", ""))
def test_emulation_passes_the_gpu_checks(op, case):
    inp = B.build(op, case)
    ref, worst, fails = B.verify(op, inp, B.OPS[op][3](inp), B.K_FAMILY[op])
    WORST[op] = max(WORST.get(op, 0.0), worst)
    for k, n in ref.note.items():
        NOTES[f"{op}: {k}"] = NOTES.get(f"{op}: {k}", 0) + n
    print(f"\n[{op} {case}] worst |emulation - ref| / (U absref) = {worst:.3g}; {ref.note}")
    assert not fails, fails


@pytest.mark.parametrize("mutant", list(B.MUTANTS))
def test_mutant_of_the_emulation_fails_the_gpu_checks(mutant):
    caught = {}
    for op in B.MUTANTS[mutant]:
        for case in B.OPS[op][1]:
            if B.is_big(op, case):
                continue                                             # (small cases only)
            inp = B.build(op, case)
            if inp.get("einval") or inp.get("ecap"):
                continue
            _, _, fails = B.verify(op, inp, B.OPS[op][3](inp, mutant), B.K_FAMILY[op])
            if fails:
                caught.setdefault(op, []).append(case)
    CAUGHT[mutant] = caught
    print(f"\n[{mutant}] caught by", caught)
    assert set(caught) == set(B.MUTANTS[mutant]), f"mutant `{mutant}` survives on {set(B.MUTANTS[mutant]) - set(caught)}"


def test_the_report():
    """the emulation's worst ratio per family (what seeded K_FAMILY before the GPU run), the census and the cases that catch each mutant"""
    print("\nworst ratio of the emulation per family:", {k: round(v, 4) for k, v in sorted(WORST.items())})
    print("roundings, decisions and subnormal values:", NOTES)
    for m, c in CAUGHT.items():
        print(f"{m}: " + "; ".join(f"{op}: {', '.join(cs)}" for op, cs in c.items()))
    assert set(WORST) <= set(B.K_FAMILY)
    assert not any(n for k, n in NOTES.items() if k.endswith("subnormal values")), NOTES
