"""The bf16 entry points of the tiny-MLP engine (csrc/mlp_bf16.hip, the bf16 modes of csrc/mlp.hip and csrc/tone_wgrad.hip) against the
float64 restatement in mlp_bf16_ref64.py -- never against another kernel, and through the C entry points only (weights go through
esr_mlp_pack_bf16 or esr_mlp_pack_batch with packed16, so the weight rounding and both operand permutations are under test):
  esr_mlp_fwd_bf16  esr_mlp_fwd_fine_bf16 (X, X16, X16 with X = NULL)  esr_mlp_dgrad_bf16  esr_mlp_dgrad_fine_bf16  esr_mlp_wgrad_bf16
  esr_mlp_wgrad_batch (bf16_operands = 1, with and without X16 on the job)  esr_tone_wgrad_recompute_bf16

Per fp32 value: |gpu - ref| <= K * 2^-24 * absref + FLOOR; per stored bf16 value: inside [r16(ref - d), r16(ref + d)], bit equality
where the ends coincide (mlp_bf16_ref64's docstring); every layer behind a stored tile is judged on the device's own tile, and every
case end to end as well.  On top: the padding rows of z and the dX rows without a reference column are exactly 0, dZ is exactly 0 where
its mask bit is 0, mask bit == (stored H > 0), tiles outside the range, unsaved H / M, a NULL dZ[l]'s neighbours and every output of a
call that returns ESR_EINVAL / ESR_ECAP keep their prefill bits, the X16 forward equals the X forward bit for bit.  Everything is
finite, every buffer -- the half-size bf16 tiles included -- carries a guard that must come back bit-identical, every input comes back
bit-identical.  The input sets are mlp_bf16_ref64's (shared with the host test).  One chained case per kind runs forward -> input
gradients -> weight gradients on the device's own M, H and dZ.  The cases marked big take a second trip through the 256 workgroups of
8 tiles.  The last test prints, under -s, the worst ratio per family, the ambiguous roundings, the mask flips and the subnormal census."""
import ctypes as C

import pytest
import torch

import mlp_bf16_ref64 as B
import mlp_ref64 as R
from test_gpu_mlp_ref64 import DEV, GUARD, Bufs, _L

pytestmark = pytest.mark.gpu

K_FAMILY = B.K_FAMILY           # per family, with the measured worst ratios: mlp_bf16_ref64.py
WORST, NOTES = {}, {}


class Packed16:
    """one net on the device: the reference tensors, esr_mlp_pack's buffer (biases) and the bf16 twin; `batch`: both from one
    esr_mlp_pack_batch launch, else esr_mlp_pack + esr_mlp_pack_bf16"""
    def __init__(self, b, kind, Ws, Bs, batch):
        lib, L, s = _L()
        self.kind, self.W, self.B = kind, [b.inp(w) for w in Ws], [b.inp(x) for x in Bs]
        self.w = lib.EsrMlpWeights()
        for i in range(len(Ws)):
            self.w.w[i], self.w.b[i] = self.W[i].data_ptr(), self.B[i].data_ptr()
        self.p32 = torch.full((L.esr_mlp_packed_floats(kind),), 7.0, device=DEV)
        n16 = L.esr_mlp_packed_bf16_elems(kind)
        self.buf16 = torch.full((n16 + GUARD,), 7.0, dtype=torch.bfloat16, device=DEV)
        self.p16 = self.buf16[:n16]
        if batch:
            kinds, ws = (C.c_int32 * 1)(kind), (C.c_void_p * 1)(C.addressof(self.w))
            p32s, p16s = (C.c_void_p * 1)(self.p32.data_ptr()), (C.c_void_p * 1)(self.p16.data_ptr())
            lib.check(L.esr_mlp_pack_batch(1, kinds, ws, p32s, p16s, None, s), "mlp_pack_batch")
        else:
            lib.check(L.esr_mlp_pack(kind, C.byref(self.w), lib.ptr(self.p32), s), "mlp_pack")
            lib.check(L.esr_mlp_pack_bf16(kind, C.byref(self.w), lib.ptr(self.p16), s), "mlp_pack_bf16")

    def guard_ok(self):
        return bool((self.buf16[self.p16.numel():] == 7).all())


def _fwd_launch(inp, nets, X, X16, H, M, z):
    lib, L, s = _L()
    pa, p = lib.ptr_array, lib.ptr
    n0, ein = nets[0], inp["einval"]
    if inp["entry"] == "fine":
        n1 = nets[1]
        Xa = None if (inp["fmt"] == "X16only" or ein == "no_input") else X
        return L.esr_mlp_fwd_fine_bf16(p(n0.p32), p(n0.p16), p(n1.p32), p(n1.p16), p(Xa), p(None if ein == "no_input" else X16), inp["t_on"],
                                       inp["T"], pa(H), pa(M), inp["crow"], p(z["z_off"]), p(z["z_emo"]), s)
    kind = 7 if ein == "bad_kind" else inp["kind"]
    return L.esr_mlp_fwd_bf16(kind, p(n0.p32), p(n0.p16), p(X), inp["t0"], inp["t1"], pa(H), pa(M), inp["save"], inp["crow"], p(z["z"]), s)


def run_fwd(inp):
    lib, L, s = _L()
    b = Bufs()
    nets = [Packed16(b, inp["kind"], Ws, Bs, batch=(inp["entry"] == "fine")) for Ws, Bs in inp["nets"]]
    X = b.inp(inp["X"])
    X16 = b.inp(inp["X16"]) if "X16" in inp else None
    fill = B._fwd_fill(inp)
    nh = R.NETS[inp["kind"]].nl - 1
    outs = {k: b.out(k, v) for k, v in fill.items()}
    H, M = [outs[f"H{l}"] for l in range(nh)], [outs[f"M{l}"] for l in range(nh)]
    rc = _fwd_launch(inp, nets, X, X16, H, M, {k: outs[k] for k in inp["znames"]})
    if inp["einval"]:
        assert rc == R.ESR_EINVAL, rc
    else:
        lib.check(rc, "mlp_fwd_bf16")
    got = b.collect()
    assert all(n.guard_ok() for n in nets), "the guard behind a packed bf16 buffer changed"
    return got


def _dgrad_launch(inp, nets, dz, M, dZ, dX):
    lib, L, s = _L()
    pa, p = lib.ptr_array, lib.ptr
    if inp["entry"] == "fine":
        return L.esr_mlp_dgrad_fine_bf16(p(nets[0].p16), p(nets[1].p16), p(dz), inp["t_on"], inp["T"], pa(M), pa(dZ), p(dX), s)
    return L.esr_mlp_dgrad_bf16(inp["kind"], p(nets[0].p16), p(dz), inp["t0"], inp["t1"], pa(M), pa(dZ), p(dX), s)


def run_dgrad(inp):
    """returns (inputs as verified, outputs, chained weight gradient); a chained case takes the masks from the device's own forward
    and hands its H and dZ tiles on to the weight gradient"""
    lib, L, s = _L()
    b = Bufs()
    net = R.NETS[inp["kind"]]
    nets = [Packed16(b, inp["kind"], Ws, Bs, batch=(inp["entry"] == "fine")) for Ws, Bs in inp["nets"]]
    nh = net.nl - 1
    Hdev = None
    if inp["chained"]:
        fcfg = dict(inp, entry="fwd", save=1, crow=0, znames={"z": inp["T"]}, einval=None, fmt="X")
        ffill = B._fwd_fill(fcfg)
        Hdev = [ffill[f"H{l}"].to(DEV) for l in range(nh)]
        Mdev = [ffill[f"M{l}"].to(DEV) for l in range(nh)]
        lib.check(_fwd_launch(fcfg, nets, b.inp(inp["X"]), None, Hdev, Mdev, {"z": ffill["z"].to(DEV)}), "mlp_fwd_bf16 (chained)")
        torch.cuda.synchronize()
        inp = dict(inp, M=[m.cpu() for m in Mdev])
    dz = b.inp(inp["dz"])
    M = [b.inp(m) for m in inp["M"]]
    outs = {k: b.out(k, v) for k, v in B._dg_fill(inp).items()}
    dZ = [None if inp["null"] == l else outs[f"dZ{l}"] for l in range(nh)]
    lib.check(_dgrad_launch(inp, nets, dz, M, dZ, outs["dX"]), "mlp_dgrad_bf16")
    got = b.collect()
    extra = None
    if inp["chained"]:
        job = dict(kind=inp["kind"], crow=0, t0=inp["t0"], t1=inp["t1"], X=inp["X"], H=[h.cpu() for h in Hdev],
                   dZ=[got[f"dZ{l}"] for l in range(nh)], dz=inp["dz"],
                   gw0=[torch.full((net.dims[l + 1], net.dims[l]), 0.25) for l in range(net.nl)],
                   gb0=[torch.full((net.dims[l + 1],), -0.5) for l in range(net.nl)])
        winp = dict(op="wgrad", name=inp["name"], J=[job], ecap=False, batch=False, x16=False)
        extra = (winp, run_wgrad(winp))
    return inp, got, extra


def run_wgrad(inp):
    lib, L, s = _L()
    b = Bufs()
    keep, jobs = [], (lib.EsrWgradJob * len(inp["J"]))()
    single = None
    for j, job in enumerate(inp["J"]):
        net = R.NETS[job["kind"]]
        X16 = b.inp(job["X16"]) if "X16" in job else None
        # (with X16 on the job X is not read: a one-job call hands over a tile of 1000s in its place)
        X = b.inp(torch.full_like(job["X"], 1e3) if X16 is not None and len(inp["J"]) == 1 else job["X"])
        dz = b.inp(job["dz"])
        H, dZ = [b.inp(h) for h in job["H"]], [b.inp(z) for z in job["dZ"]]
        gw = [b.out(f"gw{j}_{l}", job["gw0"][l]) for l in range(net.nl)]
        gb = [b.out(f"gb{j}_{l}", job["gb0"][l]) for l in range(net.nl)]
        arrs = [lib.ptr_array(t) for t in (H, dZ, gw, gb)]
        keep.append(arrs)
        J = jobs[j]
        J.kind, J.color_row0, J.t0, J.t1 = job["kind"], job["crow"], job["t0"], job["t1"]
        J.X, J.dz = X.data_ptr(), dz.data_ptr()
        J.H, J.dZ, J.gw, J.gb = [C.addressof(a) for a in arrs]
        J.X16, J.amax = None if X16 is None else X16.data_ptr(), None
        single = (job, X, dz, arrs)
    n = 8 if inp["ecap"] else L.esr_mlp_wgrad_scratch_floats()
    scratch = torch.full((n + GUARD,), 7.0, device=DEV)
    if len(inp["J"]) == 1 and not inp["batch"]:
        job, X, dz, (H, dZ, gw, gb) = single
        rc = L.esr_mlp_wgrad_bf16(job["kind"], lib.ptr(X), job["crow"], H, dZ, lib.ptr(dz), job["t0"], job["t1"], gw, gb, lib.ptr(scratch),
                                  C.c_int64(n), s)
    else:
        rc = L.esr_mlp_wgrad_batch(jobs, len(inp["J"]), 1, lib.ptr(scratch), C.c_int64(n), s)
    if inp["ecap"]:
        assert rc == R.ESR_ECAP, rc
    else:
        lib.check(rc, "mlp_wgrad_bf16")
    got = b.collect()
    assert bool((scratch[n:] == 7).all()), "the guard behind the scratch changed"
    return got


def run_tone(inp):
    lib, L, s = _L()
    b = Bufs()
    p = lib.ptr
    Xt, dzt, W0, b0, W1 = [b.inp(inp[k]) for k in ("Xt", "dzt", "W0", "b0", "W1")]
    o = {k: b.out(k, v) for k, v in inp["pre"].items()}
    n = L.esr_tone_wgrad_scratch_floats()
    scratch = torch.full((n + GUARD,), 7.0, device=DEV)
    lib.check(L.esr_tone_wgrad_recompute_bf16(p(Xt), p(dzt), p(W0), p(b0), p(W1), inp["t0"], inp["T"], p(o["gw0"]), p(o["gb0"]), p(o["gw1"]),
                                              p(o["gb1"]), p(scratch), C.c_int64(n), s), "tone_wgrad_recompute_bf16")
    got = b.collect()
    assert bool((scratch[n:] == 7).all()), "the guard behind the scratch changed"
    return got


def _record(op, case, ref, worst):
    WORST[op] = max(WORST.get(op, 0.0), worst)
    for k, n in ref.note.items():
        NOTES[f"{op}: {k}"] = NOTES.get(f"{op}: {k}", 0) + n
    print(f"\n[{op} {case}] worst |gpu - ref| / (U absref) = {worst:.3g} (K = {K_FAMILY[op]}); {ref.note or ''}")


@pytest.mark.parametrize("op,case", B.all_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_kernel_against_the_float64_restatement(op, case):
    assert set(B.ENTRY_POINTS) == set(B.OPS)
    inp = B.build(op, case)
    extra = None
    try:
        if inp["op"] == "fwd":
            got = run_fwd(inp)
        elif inp["op"] == "dgrad":
            inp, got, extra = run_dgrad(inp)
        elif inp["op"] == "wgrad":
            got = run_wgrad(inp)
        else:
            got = run_tone(inp)
    except RuntimeError as e:                                         # a device error ends the file: nothing more is started on that card
        pytest.exit(f"{op} {case}: {e}", returncode=3)
    ref, worst, fails = B.verify(op, inp, got, K_FAMILY[op])
    _record(op, case, ref, worst)
    if extra is not None:                                             # the chained case's weight gradients, from the device's H and dZ
        wref, wworst, wfails = B.verify("wgrad_bf16", extra[0], extra[1], K_FAMILY["wgrad_bf16"])
        _record("wgrad_bf16", case, wref, wworst)
        fails = fails + wfails
    assert not fails, fails


@pytest.mark.parametrize("x_case,x16_case", B.X16_TWINS)
def test_the_x16_forward_equals_the_x_forward_bit_for_bit(x_case, x16_case):
    try:
        a, b = run_fwd(B.case_fwd(x_case)), run_fwd(B.case_fwd(x16_case))
    except RuntimeError as e:
        pytest.exit(f"{x_case} / {x16_case}: {e}", returncode=3)
    assert set(a) == set(b)
    for k in a:
        assert R.same_bits(a[k], b[k]), k


def test_the_report():
    """the worst ratio per family, the ambiguous roundings, the mask flips and the subnormal census (printed under -s)"""
    print("\nworst ratio per family:", {k: round(v, 4) for k, v in sorted(WORST.items())})
    print("roundings, mask flips, decisions and subnormal values:", NOTES)
    assert set(WORST) <= set(K_FAMILY)
    assert not any(n for k, n in NOTES.items() if k.endswith("subnormal values")), NOTES
