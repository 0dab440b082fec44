"""The DVGO pre-stage entry points of csrc/dvgo.hip against the float64 restatement in dvgo_ref64.py -- never against another kernel,
and at the C ABI, not through esr_nerf_amd/dvgo.py (n_samples, NULL pointers and non-zero gradient buffers are chosen freely):
  esr_dvgo_fwd  esr_dvgo_eval  esr_dvgo_bwd  esr_dvgo_count  esr_dvgo_count_add

Per value: |gpu - ref| <= K * 2^-24 * absref + FLOOR (absref: dvgo_ref64's docstring), on every value of alpha, alphainv_cum (column S
included), weights, raw_rgb, rgb; depth, disp, white_bg, off_rgb, emo_rgb, on_rgb; grad_density, grad_off, grad_emo per cell; the view
sum per cell and the count.  The sample's cell is replayed bit for bit and nothing is exempted for it.  The two banded decisions (the
1e-10 clamp, taken from the kernel's own alpha; sum > 1) must be legitimate: a decision that differs from the float64 one lies inside
its band, and the share of such values stays below FLIP_CAP.  On top of the bound the bit expectations of dvgo_ref64 hold.  Every
output buffer is pre-filled (9.0, or the planted initial gradients) and carries a guard that must come back bit-identical; every
input comes back bit-identical.  The input sets are dvgo_ref64's (shared with the host test, where a binary32 emulation passes the
same checks and a list of mutants does not).  The worst ratio per operation is printed under -s."""
import ctypes as C

import pytest
import torch

import dvgo_ref64 as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 8
K_FAMILY = R.K_FAMILY
WORST, FLIPS = {}, {}


def _L():
    from esr_nerf_amd import _lib
    return _lib, _lib.lib(), _lib.stream_ptr(DEV)


class Bufs:
    """device copies of the inputs (checked unchanged afterwards) and guarded, pre-filled output buffers"""
    def __init__(self):
        self.ins, self.outs = [], {}

    def inp(self, t):
        if t is None:
            return None
        t = t.contiguous()
        buf = torch.full((t.numel() + GUARD,), 7, dtype=t.dtype, device=DEV)
        buf[:t.numel()].copy_(t.reshape(-1))
        self.ins.append((t, buf))
        return buf[:t.numel()]

    def out(self, name, shape, init=9.0):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + GUARD,), 7, dtype=torch.float32, device=DEV)
        if torch.is_tensor(init):
            buf[:n].copy_(init.reshape(-1))
        else:
            buf[:n].fill_(init)
        self.outs[name] = (buf, n, tuple(shape))
        return buf[:n]

    def collect(self):
        torch.cuda.synchronize()
        for host, buf in self.ins:
            assert R.same_bits(buf[:host.numel()].cpu(), host.reshape(-1)), "an input buffer changed"
            assert bool((buf[host.numel():] == 7).all()), "the guard of an input buffer changed"
        got = {}
        for name, (buf, n, shape) in self.outs.items():
            assert bool((buf[n:] == 7).all()), f"{name}: the guard changed"
            got[name] = buf[:n].cpu().reshape(shape)
        return got


def _p(lib, t):
    return 0 if t is None else (lib.ptr(t).value or 0)


def _model(lib, b, i):
    dens, off, emo = (b.inp(i.get(k)) for k in ("density", "off_color", "emo_color"))
    return lib.EsrDvgo(_p(lib, dens), _p(lib, off), _p(lib, emo), (C.c_int32 * 3)(*i["dims"]), (C.c_float * 3)(*i["lo"].tolist()),
                       (C.c_float * 3)(*i["hi"].tolist()), i["near"], i["far"], i["step_scale"], i["interval"], i["act_shift"], i["S"])


def _rays(lib, b, i):
    f = R.full_rays(i)
    o, d = b.inp(f["rays_o"]), b.inp(f["rays_d"])
    nrm, jit, em = b.inp(R.ray_norm(f["rays_d"])), b.inp(f["jitter"]), b.inp(f["em_modes"])
    return lib.EsrDvgoRays(_p(lib, o), _p(lib, d), _p(lib, nrm), _p(lib, jit), _p(lib, em), i["em_all"], o.shape[0] // 3), f, o.shape[0] // 3


TRAIN_OUT = lambda n, S: dict(alpha=(n, S), alphainv_cum=(n, S + 1), weights=(n, S), raw_rgb=(n, S, 3), rgb=(n, 3))
EVAL_OUT = lambda n, S: dict(alpha=(n, S), depth=(n,), disp=(n,), white_bg=(n,), off_rgb=(n, 3), on_rgb=(n, 3), emo_rgb=(n, 3))


def _forward(i, evaluate, b=None):
    lib, L, s = _L()
    b = b or Bufs()
    P = _model(lib, b, i)
    Rr, f, n = _rays(lib, b, i)
    outs = {k: b.out(k, shape) for k, shape in (EVAL_OUT if evaluate else TRAIN_OUT)(n, i["S"]).items()}
    O = lib.EsrDvgoOut(**{k: _p(lib, v) for k, v in outs.items()})
    entry = L.esr_dvgo_eval if evaluate else L.esr_dvgo_fwd
    lib.check(entry(C.byref(P), C.byref(Rr), C.byref(O), s), "esr_dvgo_eval" if evaluate else "esr_dvgo_fwd")
    return b, P, Rr, f, outs


def run_fwd(i):
    return _forward(i, False)[0].collect()


def run_eval(i):
    return _forward(i, True)[0].collect()


def run_bwd(i):
    lib, L, s = _L()
    b, P, Rr, f, outs = _forward(i, False)
    ups = [b.inp(f[k]) for k in ("g_alphainv_cum", "g_weights", "g_raw_rgb", "g_rgb")]
    grads = [b.out(k, tuple(i["grad0"][k].shape), i["grad0"][k]) for k in R.GRAD_NAMES]
    nulls = [b.out("null_" + k, tuple(i["grad0"][k].shape), i["grad0"][k]) for k in R.GRAD_NAMES]
    fw = [_p(lib, outs[k]) for k in ("alpha", "alphainv_cum", "raw_rgb")]
    B = lib.EsrDvgoBwd(*fw, *[_p(lib, u) for u in ups], *[_p(lib, g) for g in grads])
    lib.check(L.esr_dvgo_bwd(C.byref(P), C.byref(Rr), C.byref(B), s), "esr_dvgo_bwd")
    B0 = lib.EsrDvgoBwd(*fw, 0, 0, 0, 0, *[_p(lib, g) for g in nulls])
    lib.check(L.esr_dvgo_bwd(C.byref(P), C.byref(Rr), C.byref(B0), s), "esr_dvgo_bwd")
    return b.collect()


def run_count(i):
    lib, L, s = _L()
    b = Bufs()
    P = _model(lib, b, i)
    Rr, f, n = _rays(lib, b, i)
    total = b.out("sum", i["dims"], i["sum0"])
    count = b.out("count", i["dims"], i["count0"])
    lib.check(L.esr_dvgo_count(C.byref(P), C.byref(Rr), lib.ptr(total), s), "esr_dvgo_count")
    lib.check(L.esr_dvgo_count_add(lib.ptr(total), C.c_int64(total.numel()), lib.ptr(count), s), "esr_dvgo_count_add")
    return b.collect()


RUN = {"dvgo_fwd": run_fwd, "dvgo_eval": run_eval, "dvgo_bwd": run_bwd, "dvgo_count": run_count}


@pytest.mark.parametrize("op,case", R.all_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_kernel_against_the_float64_restatement(op, case):
    assert set(RUN) == set(R.OPS)
    inp = R.build(op, case)
    try:
        got = RUN[op](inp)
    except RuntimeError as e:                                         # a device error ends the file: nothing more is started on that card
        pytest.exit(f"{op} {case}: {e}", returncode=3)
    fam = R.OPS[op][4]
    ref, worst, fails = R.verify(op, inp, got, K_FAMILY[fam])
    WORST[op] = max(WORST.get(op, 0.0), worst)
    FLIPS[op] = FLIPS.get(op, 0) + sum(ref.flips.values())
    print(f"\n[{op} {case}] worst |gpu - ref| / (U absref) = {worst:.3g} (K = {K_FAMILY[fam]}); flips {ref.flips}, share {ref.share:.3g}; "
          f"census: {sorted(inp['census'])}")
    assert not fails, fails
    assert ref.share <= R.FLIP_CAP
    assert inp["claims"] <= inp["census"], inp["claims"] - inp["census"]


def test_a_call_without_rays_touches_nothing():
    lib, L, s = _L()
    i = dict(R.build("dvgo_bwd", "lattice_S2_n3"))
    b = Bufs()
    P = _model(lib, b, i)
    Rr = lib.EsrDvgoRays(0, 0, 0, 0, 0, 0, 0)
    outs = {k: b.out(k, shape) for k, shape in {**TRAIN_OUT(3, 2), **EVAL_OUT(3, 2)}.items()}
    O = lib.EsrDvgoOut(**{k: _p(lib, v) for k, v in outs.items()})
    lib.check(L.esr_dvgo_fwd(C.byref(P), C.byref(Rr), C.byref(O), s), "esr_dvgo_fwd")
    lib.check(L.esr_dvgo_eval(C.byref(P), C.byref(Rr), C.byref(O), s), "esr_dvgo_eval")
    grads = [b.out(k, tuple(i["grad0"][k].shape), i["grad0"][k]) for k in R.GRAD_NAMES]
    B = lib.EsrDvgoBwd(*[_p(lib, outs[k]) for k in ("alpha", "alphainv_cum", "raw_rgb")], 0, 0, 0, 0, *[_p(lib, g) for g in grads])
    lib.check(L.esr_dvgo_bwd(C.byref(P), C.byref(Rr), C.byref(B), s), "esr_dvgo_bwd")
    total = b.out("sum", i["dims"], 0.25)
    lib.check(L.esr_dvgo_count(C.byref(P), C.byref(Rr), lib.ptr(total), s), "esr_dvgo_count")
    count = b.out("count", i["dims"], 3.0)
    lib.check(L.esr_dvgo_count_add(lib.ptr(total), C.c_int64(0), lib.ptr(count), s), "esr_dvgo_count_add")
    got = b.collect()
    for k in outs:
        assert bool((got[k] == 9.0).all()), k
    for k in R.GRAD_NAMES:
        assert R.same_bits(got[k], i["grad0"][k]), k
    assert bool((got["sum"] == 0.25).all()) and bool((got["count"] == 3.0).all())


def test_the_report():
    """the worst ratio and the banded decisions per operation (printed under -s)"""
    print("\nworst ratio per operation:", {k: round(v, 3) for k, v in sorted(WORST.items())})
    print("decisions taken against the float64 branch:", FLIPS)
    assert set(WORST) <= set(R.OPS)
