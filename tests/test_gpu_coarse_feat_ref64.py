"""The two feature entry points of csrc/coarse.hip against the float64 restatement in coarse_feat_ref64.py -- never against another
kernel, and at the C ABI, on their own (the product calls them only inside voxurfc.py's step):
  esr_coarse_feat_fwd  esr_coarse_feat_bwd

Per value: |gpu - ref| <= K * 2^-24 * absref + FLOOR (absref: coarse_feat_ref64's docstring) on all 72 rows of X and on gnorm, and per
cell on g_off_color, g_emo_color and g_grad_grid; nothing is exempted.  On top of the bound the bit expectations hold: rows 69-71 are 0,
all rows and gnorm are 0 on padding lanes, rows 12-23 are 0 on off tiles, `unit` and the view direction equal the binary32 replay, and
gradient cells without a non-zero contribution keep their planted bits.  With tiles_on = 0 the emissive pointers are NULL.  Every
output buffer is pre-filled (9.0, or the planted initial gradients) and carries a guard that must come back bit-identical; every input
comes back bit-identical.  The input sets are coarse_feat_ref64's (shared with the host test, where a binary32 emulation passes the same
checks and a list of mutants does not).  The worst ratio per operation is printed under -s."""
import ctypes as C

import pytest
import torch

import coarse_feat_ref64 as R
from test_gpu_dvgo_ref64 import Bufs

pytestmark = pytest.mark.gpu

K_FAMILY = R.K_FAMILY
WORST = {}


def _L():
    from esr_nerf_amd import _lib
    return _lib, _lib.lib(), _lib.stream_ptr("cuda")


def _scene(lib, i):
    X, Y, Z = i["dims"]
    return lib.EsrScene(xyz_min=(C.c_float * 3)(*i["lo"].tolist()), xyz_max=(C.c_float * 3)(*i["hi"].tolist()), gx=X, gy=Y, gz=Z,
                        near_=i["near"], stepdist=i["stepdist"], voxel_size=1.0)


def _forward(i):
    lib, L, s = _L()
    b = Bufs()
    f = R.full(i)
    sc = _scene(lib, i)
    T, Ton = i["T"], i["Ton"]
    geo = [b.inp(i[k]) for k in ("rays_o", "rays_d", "viewdirs")] + [b.inp(f["rec_ray"]), b.inp(f["rec_step"])]
    gg, off = b.inp(i["grad_grid"]), b.inp(i["off_color"])
    emo = None if i["null_emo"] else b.inp(i["emo_color"])
    X, gnorm = b.out("X", (T, R.XC, R.LANES)), b.out("gnorm", (T * R.LANES,))
    lib.check(L.esr_coarse_feat_fwd(C.byref(sc), *[lib.ptr(t) for t in geo], Ton, T, lib.ptr(gg), lib.ptr(off), lib.ptr(emo), lib.ptr(X),
                                    lib.ptr(gnorm), s), "esr_coarse_feat_fwd")
    return b, sc, geo, f, X, gnorm


def run_fwd(i):
    return _forward(i)[0].collect()


def run_bwd(i):
    lib, L, s = _L()
    b, sc, geo, f, X, gnorm = _forward(i)
    dO = b.inp(f["dX_off"])
    dE = None if i["null_emo"] else b.inp(f["dX_emo"])
    g = {k: (None if (k == "g_emo_color" and i["null_emo"]) else b.out(k, tuple(v.shape), v)) for k, v in i["grad0"].items()}
    lib.check(L.esr_coarse_feat_bwd(C.byref(sc), *[lib.ptr(t) for t in geo], i["Ton"], i["T"], lib.ptr(X), lib.ptr(gnorm), lib.ptr(dO),
                                    lib.ptr(dE), lib.ptr(g["g_grad_grid"]), lib.ptr(g["g_off_color"]), lib.ptr(g["g_emo_color"]), s),
              "esr_coarse_feat_bwd")
    return b.collect()


RUN = {"coarse_feat_fwd": run_fwd, "coarse_feat_bwd": run_bwd}


@pytest.mark.parametrize("op,case", R.all_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_kernel_against_the_float64_restatement(op, case):
    assert set(RUN) == set(R.OPS)
    inp = R.build(op, case)
    try:
        got = RUN[op](inp)
    except RuntimeError as e:                                         # a device error ends the file: nothing more is started on that card
        pytest.exit(f"{op} {case}: {e}", returncode=3)
    ref, worst, fails = R.verify(op, inp, got, K_FAMILY[R.OPS[op][4]])
    WORST[op] = max(WORST.get(op, 0.0), worst)
    print(f"\n[{op} {case}] worst |gpu - ref| / (U absref) = {worst:.3g} (K = {K_FAMILY[R.OPS[op][4]]}); {getattr(ref, 'note', None) or ''} census: {sorted(inp['census'])}")
    assert not fails, fails
    assert ref.share == 0 and not ref.flips                           # nothing is exempted
    assert inp["claims"] <= inp["census"], inp["claims"] - inp["census"]


def test_the_report():
    """the worst ratio per operation (printed under -s)"""
    print("\nworst ratio per operation:", {k: round(v, 3) for k, v in sorted(WORST.items())})
    assert set(WORST) <= set(R.OPS)
