"""The dense-grid entry points of csrc/adam.hip, csrc/tv.hip and csrc/dense.hip against the float64 restatement in grid_ref64.py --
never against another kernel, and through the C entry points, not the modules:
  esr_adam_step  esr_adam_step_live  esr_brick_live_from_moments  esr_tv_add_grad  esr_smooth_grad_tv_fwd  esr_smooth_grad_tv_bwd
  esr_gauss3d_fwd  esr_gauss3d_bwd  esr_central_grad_fwd  esr_central_grad_bwd

Per value: |gpu - ref| <= K * 2^-24 * absref + FLOOR (absref: grid_ref64's docstring); no value is exempted.  On top of the bound the
bit expectations of grid_ref64 hold: p', m', v' and the gradient field of the smoothed-gradient term equal the binary32 emulation
wherever every intermediate is a normal number, the error field is exactly 0 outside the mask, untouched bricks and zero-gradient
cells keep their bits, the live bytes and both counters are exact.  Everything is finite, every output buffer carries a guard
(before a pointer that is offset, and behind every buffer) that must come back bit-identical, and every input comes back
bit-identical.  Overwritten outputs are pre-filled with 9.0, accumulated ones with a pattern.  The input sets are grid_ref64's
(shared with the host test, where a binary32 emulation passes the same checks and a list of mutants does not).  The worst ratio
|gpu - ref| / (2^-24 absref) per family, the count of values the device flushed and the census are printed under -s by the last
test, from what the tests before it gathered in this process (complete only when the whole file runs in order in one process)."""
import ctypes as C

import pytest
import torch

import grid_ref64 as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 8
K_FAMILY = R.K_FAMILY           # per family, with the measured worst ratios: grid_ref64.py
WORST, NOTES, CENSUS = {}, {}, {}


def _L():
    from esr_nerf_amd import _lib
    return _lib, _lib.lib(), _lib.stream_ptr(DEV)


class Bufs:
    """device copies of the inputs (checked unchanged afterwards) and guarded output buffers; `off` shifts a buffer's pointer by
    that many elements behind a guarded head"""
    def __init__(self):
        self.ins, self.outs = [], {}

    def _place(self, n, dtype, off):
        buf = torch.full((off + n + GUARD,), 7, dtype=dtype, device=DEV)
        return buf, buf[off:off + n]

    def inp(self, t, off=0):
        if t is None:
            return None
        t = t.contiguous()
        buf, view = self._place(t.numel(), t.dtype, off)
        view.copy_(t.reshape(-1))
        self.ins.append((t, buf, view, off))
        return view

    def out(self, name, shape, init=9.0, off=0, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= s
        buf, view = self._place(n, dtype, off)
        if torch.is_tensor(init):
            view.copy_(init.reshape(-1))
        else:
            view.fill_(init)
        self.outs[name] = (buf, view, off, tuple(shape))
        return view

    def snap(self):
        torch.cuda.synchronize()
        return {name: view.cpu().reshape(shape) for name, (buf, view, off, shape) in self.outs.items()}

    def collect(self):
        got = self.snap()
        for host, buf, view, off in self.ins:
            assert R.same_bits(view.cpu(), host.reshape(-1)), "an input buffer changed"
            assert bool((buf[:off] == 7).all()) and bool((buf[off + host.numel():] == 7).all()), "the guard of an input buffer changed"
        for name, (buf, view, off, shape) in self.outs.items():
            assert bool((buf[:off] == 7).all()) and bool((buf[off + view.numel():] == 7).all()), f"{name}: the guard changed"
        return got


def _fl(v):
    return C.c_float(v)


def run_adam(i):
    lib, L, s = _L()
    b, n = Bufs(), i["n"]
    off = lambda w: 1 if i["off"] == w else 0
    p, m, v = [b.out(k, (n,), i[k], off(k)) for k in "pmv"]
    plr = b.inp(i["per_lr"], off("plr"))
    got = {}
    for k in range(R.ADAM_STEPS):
        g = b.inp(i["gs"][k], off("g"))
        lib.check(L.esr_adam_step(lib.ptr(p), lib.ptr(g), lib.ptr(m), lib.ptr(v), lib.ptr(plr), C.c_int64(n), _fl(i["lr"]),
                                  _fl(i["beta1"]), _fl(i["beta2"]), _fl(i["eps"]), _fl(i["wd"]), C.c_int32(i["step"] + k), s), "adam_step")
        got.update({f"{nm}{k + 1}": t for nm, t in b.snap().items()})
    b.collect()
    return got


def run_adam_live(i):
    lib, L, s = _L()
    b, n, nb = Bufs(), i["n"], i["nb"]
    full = R.live_full(i, DEV)
    st = {k: b.out(k, (n,), full[k]) for k in ("p", "m", "v") + tuple(f"g{t}" for t in range(R.LIVE_STEPS))}
    st["live"] = b.out("live", (nb,), full["live"], dtype=torch.uint8)
    st["per_lr"] = b.inp(i["per_lr"])
    stats = b.out("stats", (2,), torch.tensor(R.STATS0), dtype=torch.int64) if i["stats"] else None
    del full
    plan, got = R.live_plan(i), {}
    for t in range(R.LIVE_STEPS):
        before = {k: st[k].clone() for k in ("p", "m", "v", f"g{t}")}
        other = None if i["sparse"] else st[f"g{1 - t}"].clone()
        lib.check(L.esr_adam_step_live(lib.ptr(st["p"]), lib.ptr(st[f"g{t}"]), lib.ptr(st["m"]), lib.ptr(st["v"]), lib.ptr(st["per_lr"]),
                                       lib.ptr(st["live"]), n, i["lr"], i["beta1"], i["beta2"], i["eps"], i["step"] + t, i["zero_grad"],
                                       lib.ptr(stats), s), "adam_step_live")
        torch.cuda.synchronize()
        got.update(R.live_collect(i, t, plan, before, st, stats))
        assert other is None or R.same_bits(other, st[f"g{1 - t}"]), "the other step's gradient changed"
        del before
    b.collect()
    return got


def run_from_moments(i):
    lib, L, s = _L()
    b = Bufs()
    m, v = b.inp(i["m"]), b.inp(i["v"])
    live = b.out("live", (i["nb"],), i["live"], dtype=torch.uint8)
    lib.check(L.esr_brick_live_from_moments(lib.ptr(m), lib.ptr(v), i["n"], lib.ptr(live), s), "brick_live_from_moments")
    return b.collect()


def run_tv(i):
    lib, L, s = _L()
    b = Bufs()
    X, Y, Z = i["dims"]
    param = b.inp(i["param"])
    grad = b.out("grad", tuple(i["param"].shape), i["grad"])
    lib.check(L.esr_tv_add_grad(lib.ptr(param), lib.ptr(grad), _fl(i["wx"]), _fl(i["wy"]), _fl(i["wz"]), C.c_int64(X), C.c_int64(Y),
                                C.c_int64(Z), C.c_int64(i["param"].numel()), C.c_int(i["dense"]), s), "tv_add_grad")
    return b.collect()


def run_smooth_fwd(i):
    lib, L, s = _L()
    b = Bufs()
    X, Y, Z = i["dims"]
    sdf, mask = b.inp(i["sdf"]), b.inp(i["mask"])
    work = b.out("work6", (6, X, Y, Z))
    loss = b.out("loss", (1,), torch.tensor([i["loss0"]]))
    w27 = (C.c_float * 27)(*i["w"].reshape(-1).tolist())
    lib.check(L.esr_smooth_grad_tv_fwd(lib.ptr(sdf), lib.ptr(mask), w27, _fl(i["bias"]), X, Y, Z, _fl(i["voxel"]), C.c_int64(i["mc"]),
                                       _fl(i["weight"]), lib.ptr(work), lib.ptr(loss), s), "smooth_grad_tv_fwd")
    return b.collect()


def run_smooth_bwd(i):
    lib, L, s = _L()
    b = Bufs()
    X, Y, Z = i["dims"]
    work, go = b.inp(i["work6"]), b.inp(i["grad_out"])
    for name, g in (("grad_sdf", go), ("grad_sdf_null", None)):
        out = b.out(name, (X, Y, Z), i["grad0"])
        lib.check(L.esr_smooth_grad_tv_bwd(lib.ptr(work), X, Y, Z, _fl(i["voxel"]), C.c_int64(i["mc"]), _fl(i["weight"]), lib.ptr(g),
                                           lib.ptr(out), s), "smooth_grad_tv_bwd")
    return b.collect()


def _gauss(i, entry, src, name, init):
    lib, L, s = _L()
    b = Bufs()
    x = b.inp(i[src])
    out = b.out(name, i["dims"], init)
    w = (C.c_float * i["k"] ** 3)(*i["w"].reshape(-1).tolist())
    lib.check(getattr(L, entry)(lib.ptr(x), w, i["k"], *i["dims"], lib.ptr(out), s), entry)
    return b.collect()


def run_gauss_fwd(i):
    return _gauss(i, "esr_gauss3d_fwd", "x", "out", 9.0)


def run_gauss_bwd(i):
    return _gauss(i, "esr_gauss3d_bwd", "gout", "gin", i["gin0"])


def run_central_fwd(i):
    lib, L, s = _L()
    b = Bufs()
    sdf = b.inp(i["sdf"])
    out = b.out("grad", (*i["dims"], 3))
    lib.check(L.esr_central_grad_fwd(lib.ptr(sdf), *i["dims"], _fl(i["voxel"]), lib.ptr(out), s), "central_grad_fwd")
    return b.collect()


def run_central_bwd(i):
    lib, L, s = _L()
    b = Bufs()
    g = b.inp(i["g"])
    out = b.out("gsdf", i["dims"], i["gsdf0"])
    lib.check(L.esr_central_grad_bwd(lib.ptr(g), *i["dims"], _fl(i["voxel"]), lib.ptr(out), s), "central_grad_bwd")
    return b.collect()


RUN = {"adam_step": run_adam, "adam_live": run_adam_live, "live_from_moments": run_from_moments, "tv_add_grad": run_tv,
       "smooth_tv_fwd": run_smooth_fwd, "smooth_tv_bwd": run_smooth_bwd, "gauss3d_fwd": run_gauss_fwd, "gauss3d_bwd": run_gauss_bwd,
       "central_grad_fwd": run_central_fwd, "central_grad_bwd": run_central_bwd}


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
    WORST[fam] = max(WORST.get(fam, 0.0), worst)
    WORST[op] = max(WORST.get(op, 0.0), worst)
    for k, n in ref.note.items():
        NOTES[f"{op}: {k}"] = NOTES.get(f"{op}: {k}", 0) + n
    CENSUS.setdefault(fam, set()).update(inp["census"])
    print(f"\n[{op} {case}] worst |gpu - ref| / (U absref) = {worst:.3g} (K = {K_FAMILY[fam]}); {ref.note or ''} census: {sorted(inp['census'])}")
    assert not fails, fails
    assert ref.share == 0 and not ref.flips                           # nothing is exempted
    assert inp["claims"] <= inp["census"], inp["claims"] - inp["census"]


def test_the_report():
    """the worst ratios per family and per operation, the flushed values and the census (printed under -s)"""
    print("\nworst ratio per family:", {k: round(v, 3) for k, v in sorted(WORST.items()) if k in K_FAMILY})
    print("worst ratio per operation:", {k: round(v, 3) for k, v in sorted(WORST.items()) if k not in K_FAMILY})
    print("subnormal intermediates:", NOTES)
    for fam, c in sorted(CENSUS.items()):
        print(f"census[{fam}]:", sorted(c))
    assert set(WORST) <= set(K_FAMILY) | set(R.OPS)
