"""The f32 and split-fp16 entry points of the tiny-MLP engine (csrc/mlp.hip, csrc/mlp_split.hip, csrc/tone_wgrad.hip) against the
float64 restatement in mlp_ref64.py -- never against another kernel, every pass on inputs it is handed, and through the C entry
points only (weights go through esr_mlp_pack / esr_mlp_pack_batch, so the packing permutations and the split planes are under test):
  esr_mlp_fwd  esr_mlp_fwd_mixed  esr_mlp_fwd_fine  esr_mlp_fwd_split  esr_mlp_fwd_fine_split  esr_mlp_dgrad  esr_mlp_dgrad_fine
  esr_mlp_dgrad_split  esr_mlp_dgrad_fine_split  esr_mlp_wgrad  esr_mlp_wgrad_batch  esr_tone_wgrad_recompute
  esr_tone_wgrad_recompute_split  esr_absmax

Per value: |gpu - ref| <= K * 2^-24 * absref + FLOOR (absref: mlp_ref64's docstring); no value is exempted.  On top of the bound:
the padding rows of z and the written dX rows without a reference column are exactly 0, dZ is exactly 0 where its mask bit is 0,
tiles outside the range, unsaved H / M, dX rows above the documented count, a NULL dZ[l]'s neighbours, and every output of a call
that returns ESR_EINVAL / ESR_ECAP keep their prefill bits, `amax` and esr_absmax are exact, mask bits follow mlp_ref64's decision
rule, and the split forward leaves the range flag at 0.  Everything is finite, every output buffer carries a guard that must come
back bit-identical, every input comes back bit-identical.  Overwritten outputs are pre-filled with 9.0, accumulated ones with a
pattern the reference adds.  The input sets are mlp_ref64's (shared with the host test, where a binary32 emulation passes the same
checks and a list of mutants does not).  One chained case per kind runs forward -> input gradients -> weight gradients on the
device's own M, H and dZ.  The worst ratio per family, the mask flips and the subnormal census are printed under -s by the last test,
from what the tests before it gathered in this process."""
import ctypes as C

import pytest
import torch

import mlp_ref64 as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 8
K_FAMILY = R.K_FAMILY           # per family, with the measured worst ratios: mlp_ref64.py
WORST, NOTES = {}, {}


def _L():
    from esr_nerf_amd import _lib
    return _lib, _lib.lib(), _lib.stream_ptr(DEV)


class Bufs:
    """device copies of the inputs (checked unchanged afterwards) and guarded output buffers"""
    def __init__(self):
        self.ins, self.outs = [], {}

    def _place(self, n, dtype):
        buf = torch.full((GUARD + n + GUARD,), 7, dtype=dtype, device=DEV)
        return buf, buf[GUARD:GUARD + n]

    def inp(self, t):
        t = t.contiguous()
        buf, view = self._place(t.numel(), t.dtype)
        view.copy_(t.reshape(-1))
        self.ins.append((t, buf, view))
        return view

    def out(self, name, init):
        buf, view = self._place(init.numel(), init.dtype)
        view.copy_(init.reshape(-1))
        self.outs[name] = (buf, view, tuple(init.shape))
        return view

    def collect(self):
        torch.cuda.synchronize()
        got = {name: view.cpu().reshape(shape) for name, (buf, view, shape) in self.outs.items()}
        for host, buf, view in self.ins:
            assert R.same_bits(view.cpu(), host.reshape(-1)), "an input buffer changed"
            assert bool((buf[:GUARD] == 7).all()) and bool((buf[GUARD + host.numel():] == 7).all()), "the guard of an input buffer changed"
        for name, (buf, view, shape) in self.outs.items():
            assert bool((buf[:GUARD] == 7).all()) and bool((buf[GUARD + view.numel():] == 7).all()), f"{name}: the guard changed"
        return got


class Packed:
    """one net on the device: the reference tensors, esr_mlp_pack's buffer and (split) esr_mlp_pack_batch's planes"""
    def __init__(self, b, kind, Ws, Bs, split):
        lib, L, s = _L()
        self.kind, self.W, self.B = kind, [b.inp(w) for w in Ws], [b.inp(x) for x in Bs]
        self.w = lib.EsrMlpWeights()
        for i in range(len(Ws)):
            self.w.w[i], self.w.b[i] = self.W[i].data_ptr(), self.B[i].data_ptr()
        self.p32 = torch.full((L.esr_mlp_packed_floats(kind),), 7.0, device=DEV)
        self.planes = None
        if split:
            self.planes = torch.zeros(L.esr_mlp_packed_split_elems(kind), dtype=torch.float16, device=DEV)
            kinds, ws = (C.c_int32 * 1)(kind), (C.c_void_p * 1)(C.addressof(self.w))
            p32s, psp = (C.c_void_p * 1)(self.p32.data_ptr()), (C.c_void_p * 1)(self.planes.data_ptr())
            lib.check(L.esr_mlp_pack_batch(1, kinds, ws, p32s, None, psp, s), "mlp_pack_batch")
        else:
            lib.check(L.esr_mlp_pack(kind, C.byref(self.w), lib.ptr(self.p32), s), "mlp_pack")

    def gain(self):
        _, L, _ = _L()
        off = L.esr_mlp_split_gain_offset(self.kind)
        return self.planes[off:off + 2].view(torch.float32).cpu()


class RangeFlag:
    """the device's registered range flag (the engine's own, so later tests keep theirs): zeroed, read back, restored"""
    def __enter__(self):
        from esr_nerf_amd.fine_engine import _RANGE_FLAGS
        lib, L, _ = _L()
        if DEV not in _RANGE_FLAGS:
            _RANGE_FLAGS[DEV] = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.flag = _RANGE_FLAGS[DEV]
        lib.check(L.esr_mlp_split_range_flag(lib.ptr(self.flag)), "esr_mlp_split_range_flag")
        torch.cuda.synchronize()
        self.before = int(self.flag)
        self.flag.zero_()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.raised = int(self.flag)
        self.flag.fill_(self.before)
        return False


def _fwd_launch(inp, nets, X, H, M, z):
    lib, L, s = _L()
    pa, p = lib.ptr_array, lib.ptr
    kind, split = inp["kind"], inp["engine"] == "split"
    n0 = nets[0]
    if inp["entry"] == "fine":
        n1 = nets[1]
        if split:
            return L.esr_mlp_fwd_fine_split(p(n0.p32), p(n0.planes), p(n1.p32), p(n1.planes), p(X), inp["t_on"], inp["T"], pa(H), pa(M),
                                            inp["crow"], p(z["z_off"]), p(z["z_emo"]), s)
        return L.esr_mlp_fwd_fine(p(n0.p32), p(n1.p32), p(X), inp["t_on"], inp["T"], pa(H), pa(M), inp["crow"], p(z["z_off"]),
                                  p(z["z_emo"]), s)
    if inp["entry"] == "mixed":
        return L.esr_mlp_fwd_mixed(kind, p(n0.p32), p(X), inp["t0"], inp["t_on"], inp["t1"], pa(H), pa(M), inp["crow"], p(z["z"]), s)
    if split:
        return L.esr_mlp_fwd_split(kind, p(n0.p32), p(n0.planes), p(X), inp["t0"], inp["t1"], pa(H), pa(M), inp["save"], inp["crow"],
                                   p(z["z"]), s)
    return L.esr_mlp_fwd(kind, p(n0.p32), p(X), inp["t0"], inp["t1"], pa(H), pa(M), inp["save"], inp["crow"], p(z["z"]), s)


def run_fwd(inp):
    lib, L, s = _L()
    b = Bufs()
    split = inp["engine"] == "split"
    # (the coarse net has no split planes: its f32 buffer and a dummy stand in, the call must refuse before it reads them)
    nets = [Packed(b, inp["kind"], Ws, Bs, split and not inp["einval"]) for Ws, Bs in inp["nets"]]
    if inp["einval"]:
        nets[0].planes = torch.zeros(64, dtype=torch.float16, device=DEV)
    X = b.inp(inp["X"])
    fill = R._fwd_fill(inp)
    nh = R.NETS[inp["kind"]].nl - 1
    outs = {k: b.out(k, v) for k, v in fill.items()}
    H, M = [outs[f"H{l}"] for l in range(nh)], [outs[f"M{l}"] for l in range(nh)]
    z = {k: outs[k] for k in inp["znames"]}
    with RangeFlag() as rf:
        rc = _fwd_launch(inp, nets, X, H, M, z)
    if inp["einval"]:
        assert rc == R.ESR_EINVAL, rc
    else:
        lib.check(rc, "mlp_fwd")
        assert not split or rf.raised == 0, "the range flag was raised"
    return b.collect()


def _dgrad_launch(inp, nets, dz, M, dZ, dX, amax):
    lib, L, s = _L()
    pa, p = lib.ptr_array, lib.ptr
    kind, split = inp["kind"], inp["engine"] == "split"
    if inp["entry"] == "fine":
        if split:
            return L.esr_mlp_dgrad_fine_split(p(nets[0].planes), p(nets[1].planes), p(dz), inp["t_on"], inp["T"], pa(M), pa(dZ), p(dX),
                                              p(amax), s)
        return L.esr_mlp_dgrad_fine(p(nets[0].p32), p(nets[1].p32), p(dz), inp["t_on"], inp["T"], pa(M), pa(dZ), p(dX), s)
    if split:
        return L.esr_mlp_dgrad_split(kind, p(nets[0].planes), p(dz), inp["t0"], inp["t1"], pa(M), pa(dZ), p(dX), p(amax), s)
    return L.esr_mlp_dgrad(kind, p(nets[0].p32), p(dz), inp["t0"], inp["t1"], pa(M), pa(dZ), p(dX), s)


def run_dgrad(inp):
    """returns (inputs as verified, outputs); a chained case takes the masks from the device's own forward and hands its H, dZ on
    to the weight gradient (second result)"""
    lib, L, s = _L()
    b = Bufs()
    net = R.NETS[inp["kind"]]
    split = inp["engine"] == "split"
    nets = [Packed(b, inp["kind"], Ws, Bs, split) for Ws, Bs in inp["nets"]]
    nh = net.nl - 1
    Hdev = None
    if inp["chained"]:
        fcfg = dict(inp, entry="fwd", save=1, crow=0, znames={"z": inp["T"]})
        ffill = R._fwd_fill(fcfg)
        Hdev = [ffill[f"H{l}"].to(DEV) for l in range(nh)]
        Mdev = [ffill[f"M{l}"].to(DEV) for l in range(nh)]
        zdev = {"z": ffill["z"].to(DEV)}
        Xdev = b.inp(inp["X"])
        lib.check(_fwd_launch(fcfg, nets, Xdev, Hdev, Mdev, zdev), "mlp_fwd (chained)")
        torch.cuda.synchronize()
        inp = dict(inp, M=[m.cpu() for m in Mdev])
    dz = b.inp(inp["dz"])
    M = [b.inp(m) for m in inp["M"]]
    fill = R._dg_fill(inp)
    outs = {k: b.out(k, v) for k, v in fill.items()}
    dZ = [None if inp["null"] == l else outs[f"dZ{l}"] for l in range(nh)]
    lib.check(_dgrad_launch(inp, nets, dz, M, dZ, outs["dX"], outs.get("amax")), "mlp_dgrad")
    got = b.collect()
    if split:
        for ni, a, e in inp["segs"]:
            if e > a:
                got[f"G{ni}"] = nets[ni].gain()
    extra = None
    if inp["chained"]:
        job = dict(kind=inp["kind"], crow=0, t0=inp["t0"], t1=inp["t1"], X=inp["X"], H=[h.cpu() for h in Hdev],
                   dZ=[got[f"dZ{l}"] for l in range(nh)], dz=inp["dz"],
                   gw0=[torch.full((net.dims[l + 1], net.dims[l]), 0.25) for l in range(net.nl)],
                   gb0=[torch.full((net.dims[l + 1],), -0.5) for l in range(net.nl)])
        winp = dict(op="wgrad", engine=inp["engine"], name=inp["name"], J=[job], ecap=False, B=float(got["amax"]) if split else 0.0)
        extra = (winp, run_wgrad(winp))
    return inp, got, extra


def run_wgrad(inp):
    lib, L, s = _L()
    b = Bufs()
    split = inp["engine"] == "split"
    keep, jobs = [], (lib.EsrWgradJob * len(inp["J"]))()
    amax = b.inp(torch.tensor([inp["B"]])) if split else None
    single = None
    for j, job in enumerate(inp["J"]):
        net = R.NETS[job["kind"]]
        X, dz = b.inp(job["X"]), b.inp(job["dz"])
        H, dZ = [b.inp(h) for h in job["H"]], [b.inp(z) for z in job["dZ"]]
        gw = [b.out(f"gw{j}_{l}", job["gw0"][l]) for l in range(net.nl)]
        gb = [b.out(f"gb{j}_{l}", job["gb0"][l]) for l in range(net.nl)]
        arrs = [lib.ptr_array(t) for t in (H, dZ, gw, gb)]
        keep.append(arrs)
        J = jobs[j]
        J.kind, J.color_row0, J.t0, J.t1 = job["kind"], job["crow"], job["t0"], job["t1"]
        J.X, J.dz = X.data_ptr(), dz.data_ptr()
        J.H, J.dZ, J.gw, J.gb = [C.addressof(a) for a in arrs]
        J.X16, J.amax = None, amax.data_ptr() if split else None
        single = (job, X, dz, arrs)
    n = 8 if inp["ecap"] else L.esr_mlp_wgrad_scratch_floats()
    scratch = torch.full((n + GUARD,), 7.0, device=DEV)
    if len(inp["J"]) == 1 and not split and not inp.get("batch"):
        job, X, dz, (H, dZ, gw, gb) = single
        rc = L.esr_mlp_wgrad(job["kind"], lib.ptr(X), job["crow"], H, dZ, lib.ptr(dz), job["t0"], job["t1"], gw, gb, lib.ptr(scratch),
                             C.c_int64(n), s)
    else:
        rc = L.esr_mlp_wgrad_batch(jobs, len(inp["J"]), 0, lib.ptr(scratch), C.c_int64(n), s)
    if inp["ecap"]:
        assert rc == R.ESR_ECAP, rc
    else:
        lib.check(rc, "mlp_wgrad")
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
    if inp["engine"] == "split":
        amax = b.inp(torch.tensor([inp["B"]]))
        rc = L.esr_tone_wgrad_recompute_split(p(Xt), p(dzt), p(W0), p(b0), p(W1), p(amax), inp["t0"], inp["T"], p(o["gw0"]), p(o["gb0"]),
                                              p(o["gw1"]), p(o["gb1"]), p(scratch), C.c_int64(n), s)
    else:
        rc = L.esr_tone_wgrad_recompute(p(Xt), p(dzt), p(W0), p(b0), p(W1), inp["t0"], inp["T"], p(o["gw0"]), p(o["gb0"]), p(o["gw1"]),
                                        p(o["gb1"]), p(scratch), C.c_int64(n), s)
    lib.check(rc, "tone_wgrad_recompute")
    got = b.collect()
    assert bool((scratch[n:] == 7).all()), "the guard behind the scratch changed"
    return got


def run_absmax(inp):
    lib, L, s = _L()
    n = inp["x"].numel()
    x = torch.full((4 + n + GUARD,), 1e9, device=DEV)                   # (the entry wants 16-byte alignment: a float4 of guard)
    x[4:4 + n] = inp["x"].to(DEV)
    b = Bufs()
    out = b.out("out", torch.tensor([inp["pre"]]))
    lib.check(L.esr_absmax(lib.ptr(x[4:4 + n]), C.c_int64(n), lib.ptr(out), s), "absmax")
    got = b.collect()
    assert R.same_bits(x[4:4 + n].cpu(), inp["x"]) and bool((x[:4] == 1e9).all()) and bool((x[4 + n:] == 1e9).all())
    return got


def _record(op, case, fam, ref, worst):
    WORST[fam] = max(WORST.get(fam, 0.0), worst)
    WORST[op] = max(WORST.get(op, 0.0), worst)
    for k, n in ref.note.items():
        NOTES[f"{fam}: {k}"] = NOTES.get(f"{fam}: {k}", 0) + n
    print(f"\n[{op} {case}] worst |gpu - ref| / (U absref) = {worst:.3g} (K = {K_FAMILY[fam]}); {ref.note or ''}")


@pytest.mark.parametrize("op,case", R.all_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_kernel_against_the_float64_restatement(op, case):
    assert set(R.ENTRY_POINTS) == set(R.OPS)
    inp = R.build(op, case)
    extra = None
    try:
        if inp["op"] == "fwd":
            got = run_fwd(inp)
        elif inp["op"] == "dgrad":
            inp, got, extra = run_dgrad(inp)
        elif inp["op"] == "wgrad":
            got = run_wgrad(inp)
        elif inp["op"] == "tone":
            got = run_tone(inp)
        else:
            got = run_absmax(inp)
    except RuntimeError as e:                                         # a device error ends the file: nothing more is started on that card
        pytest.exit(f"{op} {case}: {e}", returncode=3)
    fam = R.OPS[op][4]
    ref, worst, fails = R.verify(op, inp, got, K_FAMILY[fam])
    _record(op, case, fam, ref, worst)
    if extra is not None:                                             # the chained case's weight gradients, from the device's H and dZ
        wop = "wgrad_" + inp["engine"]
        wref, wworst, wfails = R.verify(wop, extra[0], extra[1], K_FAMILY[wop])
        _record(wop, case, wop, wref, wworst)
        fails = fails + wfails
    assert not fails, fails


def test_the_report():
    """the worst ratios per family and per operation, the mask flips and the subnormal census (printed under -s)"""
    print("\nworst ratio per family:", {k: round(v, 4) for k, v in sorted(WORST.items()) if k in K_FAMILY})
    print("worst ratio per operation:", {k: round(v, 4) for k, v in sorted(WORST.items()) if k not in K_FAMILY})
    print("mask flips, decisions and subnormal values:", NOTES)
    assert set(WORST) <= set(K_FAMILY) | set(R.OPS)
