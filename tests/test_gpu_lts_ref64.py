"""The arithmetic entry points of csrc/lts.hip against the float64 restatement in lts_ref64.py -- never against another kernel:
  esr_expgrad_fwd  esr_expgrad_bwd  esr_lts_dirs  esr_lts_dirs_rays  esr_lts_combine_fwd  esr_lts_combine_bwd  esr_emit_edit

Per value: |gpu - ref| <= K * 2^-24 * absref + FLOOR (absref: lts_ref64's docstring).  Zero-mask slots (rec_ray = -1 rows, d_emission
on certain points) are exactly 0, everything is finite, every output buffer carries a guard tail that must come back bit-identical,
the inputs come back bit-identical, and the grid cells no sample touches keep their pre-fill exactly.  Overwritten outputs are
pre-filled with 9.0, accumulated ones with a pattern.  The input sets are lts_ref64's (shared with the host test, where a binary32
emulation passes the same bounds and a list of mutants does not); each case asserts the census of the classes it claims.  The worst
ratio |gpu - ref| / (2^-24 absref) per family, the decision flips and the census are printed under -s by the last test, from what
the tests before it gathered in this process (complete only when the whole file runs in order in one process)."""
import ctypes as C

import pytest
import torch

import lts_ref64 as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 8
K_FAMILY = R.K_FAMILY           # per family, with the measured worst ratios: lts_ref64.py
WORST, FLIPS, CENSUS = {}, {}, {}


def _L():
    from esr_nerf_amd import _lib
    return _lib, _lib.lib(), _lib.stream_ptr(DEV)


class Bufs:
    """device copies of the inputs (checked unchanged afterwards) and guarded output buffers"""
    def __init__(self):
        self.ins, self.outs = [], {}

    def inp(self, t):
        if t is None:
            return None
        d = t.to(DEV).contiguous()
        self.ins.append((t, d))
        return d

    def out(self, name, shape, init=9.0):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + GUARD,), 7.0, device=DEV)
        buf[:n] = init.to(DEV).reshape(-1) if torch.is_tensor(init) else init
        self.outs[name] = (buf, n, tuple(shape))
        return buf

    def collect(self):
        torch.cuda.synchronize()
        for host, dev in self.ins:
            assert torch.equal(dev.cpu(), host.contiguous()), "an input buffer changed"
        got = {}
        for name, (buf, n, shape) in self.outs.items():
            b = buf.cpu()
            assert bool((b[n:] == 7.0).all()), f"{name}: the guard tail changed"
            got[name] = b[:n].reshape(shape)
        return got


def _scene(i):
    from esr_nerf_amd.fine_engine import make_scene
    lo, hi = i["lo"].tolist(), i["hi"].tolist()
    return make_scene(lo, hi, lo, hi, list(i["dims"]), [32, 32, 32], i["near"], i["stepdist"], 0.25, 0.0, 1e-3, 1e-4, 20.0,
                      [0.5, 1.0, 1.5, 2.0])


def _expgrad_args(lib, b, i):
    ray = i.get("pts") is None
    t = [b.inp(i[k]) if ray else None for k in ("rays_o", "rays_d", "rec_ray", "rec_step")] + [b.inp(i.get("pts")), b.inp(i.get("noise"))]
    return [lib.ptr(x) for x in t] + [C.c_float(i["eps"])]


def run_expgrad_fwd(i):
    lib, L, s = _L()
    b, sc = Bufs(), _scene(i)
    args, sdf = _expgrad_args(lib, b, i), b.inp(i["sdf"])
    out = b.out("out", (i["n"], 4))
    lib.check(L.esr_expgrad_fwd(C.byref(sc), *args, lib.ptr(sdf), i["n"], i["zero_pad"], lib.ptr(out), s), "expgrad_fwd")
    return b.collect()


def run_expgrad_bwd(i):
    lib, L, s = _L()
    b, sc = Bufs(), _scene(i)
    args, g = _expgrad_args(lib, b, i), b.inp(i["g"])
    gs = b.out("grad_sdf", tuple(i["dims"]), i["grad0"])
    lib.check(L.esr_expgrad_bwd(C.byref(sc), *args, lib.ptr(g), i["n"], i["zero_pad"], lib.ptr(gs), s), "expgrad_bwd")
    return b.collect()


def run_lts_dirs(i):
    lib, L, s = _L()
    b = Bufs()
    raw, nrm = b.inp(i["raw"]), b.inp(i["normal"])
    P, R1 = i["P"], i["R1"]
    dirs = b.out("dirs", (P, R1, 3))
    if i.get("pts") is None:
        lib.check(L.esr_lts_dirs(lib.ptr(raw), lib.ptr(nrm), P, R1, lib.ptr(dirs), s), "lts_dirs")
    else:
        pts = b.inp(i["pts"])
        o2, d2, vr = b.out("o2", (P * (R1 - 1), 3)), b.out("d2", (P * (R1 - 1), 3)), b.out("v_rand", (P, 3))
        lib.check(L.esr_lts_dirs_rays(lib.ptr(raw), lib.ptr(nrm), lib.ptr(pts), P, R1, lib.ptr(dirs), lib.ptr(o2), lib.ptr(d2),
                                      lib.ptr(vr), s), "lts_dirs_rays")
    return b.collect()


def run_emit_edit(i):
    lib, L, s = _L()
    b = Bufs()
    m, k, c = b.inp(i["modes"]), b.inp(i["inten"]), b.inp(i["colors"])
    n = i["modes"].shape[0]
    e = b.out("emit", (n, 3), i["emit"])
    lib.check(L.esr_emit_edit(lib.ptr(e), lib.ptr(m), lib.ptr(k), lib.ptr(c), n, s), "emit_edit")
    return b.collect()


def _lts_args(lib, b, i):
    a = lib.EsrLtsArgs()
    a.n_pts, a.n_rays, a.n_sg, a.pdra_mode = i["P"], i["R"], i["J"], i["pdra"]
    for k in ("base", "rough", "metal", "normal", "view", "dirs", "off_m", "emo_m", "last2", "mus", "lambdas", "lobes", "emission"):
        setattr(a, k, b.inp(i[k]).data_ptr())
    a.umask = None if i["umask"] is None else b.inp(i["umask"]).data_ptr()
    return a


def run_lts_combine_fwd(i):
    lib, L, s = _L()
    b = Bufs()
    a = _lts_args(lib, b, i)
    oh, eh = b.out("off_hat", (2 * i["P"], 3)), b.out("emo_hat", (2 * i["P"], 3))
    lib.check(L.esr_lts_combine_fwd(C.byref(a), lib.ptr(oh), lib.ptr(eh), s), "lts_combine_fwd")
    return b.collect()


def run_lts_combine_bwd(i):
    lib, L, s = _L()
    b = Bufs()
    a = _lts_args(lib, b, i)
    P, Rr, J = i["P"], i["R"], i["J"]
    g1, g2 = b.inp(i["g_off_hat"]), b.inp(i["g_emo_hat"])
    gs = lib.EsrLtsGrads()
    shapes = dict(d_off_m=(P * Rr, 3), d_emo_m=(P * Rr, 3), d_last2=(P * Rr,), d_base=(P, 3), d_rough=(P,), d_metal=(P,),
                  d_emission=(P, 3), d_mus=(J, 3), d_lambdas=(J,), d_lobes=(J, 3))
    for k, sh in shapes.items():
        setattr(gs, k, b.out(k, sh, i[k + "0"] if k + "0" in i else 9.0).data_ptr())
    lib.check(L.esr_lts_combine_bwd(C.byref(a), lib.ptr(g1), lib.ptr(g2), C.byref(gs), s), "lts_combine_bwd")
    return b.collect()


RUN = {"expgrad_fwd": run_expgrad_fwd, "expgrad_bwd": run_expgrad_bwd, "lts_dirs": run_lts_dirs, "lts_dirs_rays": run_lts_dirs,
       "emit_edit": run_emit_edit, "lts_combine_fwd": run_lts_combine_fwd, "lts_combine_bwd": run_lts_combine_bwd}


@pytest.mark.parametrize("op,case", R.all_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_kernel_against_the_float64_restatement(op, case):
    assert set(RUN) == set(R.OPS)
    inp = R.build(op, case)
    got = RUN[op](inp)
    fam = R.OPS[op][4]
    ref, worst, fails = R.verify(op, inp, got, K_FAMILY[fam])
    WORST[fam] = max(WORST.get(fam, 0.0), worst)
    WORST[op] = max(WORST.get(op, 0.0), worst)
    for k, n in ref.flips.items():
        FLIPS[f"{op}:{k}"] = FLIPS.get(f"{op}:{k}", 0) + n
    CENSUS.setdefault(fam, set()).update(inp["census"])
    print(f"\n[{op} {case}] worst |gpu - ref| / (U absref) = {worst:.3g} (K = {K_FAMILY[fam]}); flips {ref.flips} "
          f"({ref.share:.4%}); census: {sorted(inp['census'])}")
    assert not fails, fails
    assert ref.share <= R.FLIP_CAP, f"{ref.share:.3%} of the values exempted as decision flips"
    assert inp["claims"] <= inp["census"], inp["claims"] - inp["census"]
    if op == "expgrad_bwd":                                           # cells no sample touches: bit-identical to the pre-fill
        untouched = (ref.count == 0).reshape(inp["grad0"].shape)
        assert bool(untouched.any()) or inp["n"] > 1000
        assert torch.equal(got["grad_sdf"][untouched], inp["grad0"][untouched])
    if op == "lts_dirs_rays":                                         # plain copies
        P, R1 = inp["P"], inp["R1"]
        assert torch.equal(got["o2"], inp["pts"][:, None, :].expand(P, R1 - 1, 3).reshape(-1, 3))
        assert torch.equal(got["d2"], got["dirs"][:, :R1 - 1].reshape(-1, 3)) and torch.equal(got["v_rand"], -got["dirs"][:, R1 - 1])


EXPGRAD_CLASSES = {"box corner", "face", "integer index", "outside the box", "pile of 300 in one cell", "noise", "zero_pad",
                   "second workgroup", "ray mode", "step 0", "last step", "rec_ray = -1"}
DIRS_CLASSES = {"norm 0", "dt = 0", "1e-20 magnitude", "mode 0", "mode 1", "mode 2", "mode 3", "mode 4", "hue 1.0",
                "hue on a sector boundary", "saturation 0 and 1"}
COMBINE_CLASSES = {"n_sg = 1", "n_sg = 48", "n_sg = 64", "umask NULL", "wi + wo = 0", "r2 < 1e-7 with n.h = 1",
                   "r2 on the first square above 1e-7", "lambda 0", "lambda negative", "lambda 1e3", "lobe of norm 1e-20",
                   "pre-activation above 20", "last2 = 0 on a whole wave", "one ray in the second trip", "second trip",
                   "D spans decades", "pdra certain points", "pdra uncertain points"}


def test_the_cases_reach_every_class():
    """the union of the cases' own censuses (computed on the CPU from the shared inputs) covers the issue's classes"""
    union = lambda op: set().union(*[R.build(op, c)["census"] for c in R.OPS[op][1]])
    assert EXPGRAD_CLASSES <= union("expgrad_fwd"), EXPGRAD_CLASSES - union("expgrad_fwd")
    de = union("lts_dirs") | union("emit_edit")
    assert DIRS_CLASSES <= de, DIRS_CLASSES - de
    assert COMBINE_CLASSES <= union("lts_combine_bwd"), COMBINE_CLASSES - union("lts_combine_bwd")
    assert R.MAX_SG == 64 and {c[1] for c in R.EXPGRAD_CASES.values() if c[0] == "pts"} == {1, 255, 257, 5000}
    print("\nworst ratio per family:", {k: round(v, 3) for k, v in sorted(WORST.items()) if k in K_FAMILY})
    print("worst ratio per operation:", {k: round(v, 3) for k, v in sorted(WORST.items()) if k not in K_FAMILY})
    print("decision flips:", FLIPS)
    for fam, c in sorted(CENSUS.items()):
        print(f"census[{fam}]:", sorted(c))
