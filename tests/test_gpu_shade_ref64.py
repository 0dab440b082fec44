"""Every entry point of csrc/shade.hip (but esr_sample_points, covered bit for bit elsewhere) and the two shade kernels of
csrc/coarse.hip against the float64 restatement in shade_ref64.py -- never against another kernel:
  fine tail   esr_fine_tone_in_fwd  esr_fine_tone_in_bwd  esr_fine_composite_fwd  esr_fine_composite_bwd  esr_fine_loss_fwd_bwd_dp
  LTS tail    esr_lts_tone_in_bwd  esr_composite3_fwd  esr_composite3_bwd  esr_act_fwd  esr_act_bwd  esr_act_batch
              esr_pair_loss_fwd_bwd  esr_pair_loss_batch
  coarse      esr_coarse_shade_fwd  esr_coarse_shade_bwd
  evaluation  esr_eval_aux  esr_eval_disp

Per value: |gpu - ref| <= K * 2^-24 * absref + FLOOR (absref: shade_ref64's docstring; FLOOR = 1e-30 covers binary32 underflow of
intermediates, exp(-100) and 1e-7 gradients times a sigmoid tail).  Padding rows and padding lanes are exactly 0, untouched
buffers keep their contents exactly, everything is finite.  The input sets are shade_ref64's (shared with the host test, where a
binary32 emulation passes the same bounds and a list of mutants does not); each case asserts the census of the classes it claims.
The worst ratio |gpu - ref| / (2^-24 absref) per family, the decision flips and the census are printed under -s by the last
test, from what the tests before it gathered in this process: the figures are complete only when the whole file runs in order
in one process (partial under -k or when the file is spread over workers); each case also prints its own line."""
import ctypes as C

import pytest
import torch

import shade_ref64 as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
K_FAMILY = R.K_FAMILY           # per family, with the measured worst ratios: shade_ref64.py
WORST, FLIPS, CENSUS = {}, {}, {}


def _L():
    from esr_nerf_amd import _lib
    return _lib, _lib.lib(), _lib.stream_ptr(DEV)


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _f(v):
    return C.c_float(float(v))


# ---- the launches: CPU inputs of shade_ref64 -> outputs by name ---------------------------------------------------------
def run_tone_in_fwd(i):
    lib, L, s = _L()
    T = i["tiles_all"]
    zo, ze = _d(i["z_off"]), _d(i["z_emo"])
    lin, Xt = torch.full((T, 4, 32), 9.0, device=DEV), torch.full((T, R.XT_ROWS, 32), 9.0, device=DEV)
    lib.check(L.esr_fine_tone_in_fwd(lib.ptr(zo), lib.ptr(ze), i["tiles_on"], T, lib.ptr(lin), lib.ptr(Xt), s), "tone_in_fwd")
    return dict(lin=lin, Xt=Xt)


def _tone_args(lib, i):
    keep = [_d(i[k]) for k in ("dXt", "Xt", "g_lin", "lin", "z_off", "z_emo", "rec_ray", "rec_w")]
    return keep, [lib.ptr(t) for t in keep] + [i["tiles_on"], i["tiles_all"]]


def run_tone_in_bwd(i):
    lib, L, s = _L()
    keep, args = _tone_args(lib, i)
    dz = torch.full((i["tiles_all"], 4, 32), 9.0, device=DEV)
    lib.check(L.esr_fine_tone_in_bwd(*args, lib.ptr(dz), s), "tone_in_bwd")
    return dict(dz=dz)


def run_lts_tone_in_bwd(i):
    lib, L, s = _L()
    keep, args = _tone_args(lib, i)
    dz_off, dz_emo = torch.full((i["tiles_all"], 4, 32), 9.0, device=DEV), _d(i["dz_emo0"]).clone()
    lib.check(L.esr_lts_tone_in_bwd(*args, lib.ptr(dz_off), lib.ptr(dz_emo), s), "lts_tone_in_bwd")
    return dict(dz_off=dz_off, dz_emo=dz_emo)


def run_composite_fwd(i):
    lib, L, s = _L()
    keep = [_d(i[k]) for k in ("zt", "lin", "rec_ray", "rec_w")]
    rgb = torch.full((i["tiles_all"], 4, 32), 9.0, device=DEV)
    srgb, linm = _d(i["srgb0"]).clone(), _d(i["lin0"]).clone()
    lib.check(L.esr_fine_composite_fwd(*[lib.ptr(t) for t in keep], i["tiles_all"], lib.ptr(rgb), lib.ptr(srgb), lib.ptr(linm), s),
              "composite_fwd")
    return dict(rgb=rgb, srgb_marched=srgb, lin_marched=linm)


def run_composite_bwd(i):
    lib, L, s = _L()
    keep = [_d(i[k]) for k in ("g_srgb", "g_lin", "rgb", "lin", "rec_ray", "rec_w")]
    T = i["tiles_all"]
    dw, dzt = torch.full((T * 32,), 9.0, device=DEV), torch.full((T, 4, 32), 9.0, device=DEV)
    lib.check(L.esr_fine_composite_bwd(*[lib.ptr(t) for t in keep], T, lib.ptr(dw), lib.ptr(dzt), s), "composite_bwd")
    return dict(dweight=dw, dzt=dzt)


def run_loss(i):
    lib, L, s = _L()
    keep = [_d(i[k]) for k in ("srgb_m", "lin_m", "last", "rgbs")]
    n = i["n_rays"]
    loss = _d(i["loss0"].reshape(1)).clone()
    gs, gl, ga = (torch.full(sh, 9.0, device=DEV) for sh in ((n, 3), (n, 3), (n,)))
    lib.check(L.esr_fine_loss_fwd_bwd_dp(*[lib.ptr(t) for t in keep], n, _f(i["white_bg"]), _f(i["w_lin"]), _f(i["w_ent"]),
                                         _f(i["scale"]), lib.ptr(loss), lib.ptr(gs), lib.ptr(gl), lib.ptr(ga), s), "loss")
    return dict(loss=loss, g_srgb=gs, g_lin=gl, g_last=ga)


def run_composite3_fwd(i):
    lib, L, s = _L()
    v, rr, w, out = _d(i["v"]), _d(i["rec_ray"]), _d(i["rec_w"]), _d(i["out0"]).clone()
    lib.check(L.esr_composite3_fwd(lib.ptr(v), v.shape[1], lib.ptr(rr), lib.ptr(w), i["tiles_all"], lib.ptr(out), s), "composite3_fwd")
    return dict(out=out)


def run_composite3_bwd(i):
    lib, L, s = _L()
    g, v, rr, w = _d(i["g"]), _d(i["v"]), _d(i["rec_ray"]), _d(i["rec_w"])
    dv, dw = _d(i["dv0"]).clone(), _d(i["dw0"]).clone()
    lib.check(L.esr_composite3_bwd(lib.ptr(g), lib.ptr(v), v.shape[1], lib.ptr(rr), lib.ptr(w), i["tiles_all"], i["accumulate"],
                                   lib.ptr(dv), lib.ptr(dw), s), "composite3_bwd")
    return dict(dv=dv, dweight=dw)


def run_act(i):
    lib, L, s = _L()
    z, g = _d(i["z"]), _d(i["g"])
    T, rows = z.shape[0], z.shape[1]
    fwd, bwd = torch.full_like(z, 9.0), torch.full_like(z, 9.0)
    lib.check(L.esr_act_fwd(lib.ptr(z), T, rows, i["n_ch"], i["act"], lib.ptr(fwd), s), "act_fwd")
    lib.check(L.esr_act_bwd(lib.ptr(z), lib.ptr(g), T, rows, i["n_ch"], i["act"], lib.ptr(bwd), s), "act_bwd")
    return dict(fwd=fwd, bwd=bwd)


def run_act_batch(i):
    lib, L, s = _L()
    jobs = i["jobs"]
    arr = (lib.EsrActJob * len(jobs))()
    keep, outs = [], {}
    for k, (jb, job) in enumerate(zip(arr, jobs)):
        z = _d(job["z"])
        out = torch.full_like(z, 9.0)
        keep.append(z)
        outs[f"job{k}"] = out
        jb.z, jb.out, jb.tiles, jb.rows, jb.n_ch, jb.act, jb.bwd = z.data_ptr(), out.data_ptr(), z.shape[0], z.shape[1], job["n_ch"], \
            job["act"], job["bwd"]
        for name in ("g_tile", "src", "inv", "pt1"):
            if job.get(name) is not None:
                t = _d(job[name])
                keep.append(t)
                setattr(jb, name, t.data_ptr())
        if job.get("src") is not None:
            jb.src_c, jb.n_src = job["src"].shape[1], job["src"].shape[0]
        for e, (t, c0) in enumerate(job.get("ex", [])):
            td = _d(t)
            keep.append(td)
            jb.ex[e], jb.ex_c[e], jb.ex_col0[e] = td.data_ptr(), t.shape[1], c0
    lib.check(L.esr_act_batch(arr, len(jobs), s), "act_batch")
    torch.cuda.synchronize()
    return outs


def _pair_dev(job):
    a, b, m = _d(job["a"]), _d(job.get("b")), _d(job.get("row_mask"))
    c = torch.tensor([job["count"]], dtype=torch.int32, device=DEV) if job.get("count") is not None else None
    ga = torch.full_like(a, 9.0) if job.get("want_ga", True) else None
    gb = torch.full_like(a, 9.0) if job.get("want_gb", True) else None
    return a, b, m, c, ga, gb


def run_pair_loss(i):
    lib, L, s = _L()
    a, b, m, c, ga, gb = _pair_dev(i)
    loss = _d(i["loss0"].reshape(1)).clone()
    lib.check(L.esr_pair_loss_fwd_bwd(lib.ptr(a), lib.ptr(b), C.c_int64(a.shape[0]), a.shape[1], lib.ptr(m), i["mask_value"],
                                      lib.ptr(c), i["kind"], _f(i["w_value"]), _f(i["w_a"]), _f(i["w_b"]), lib.ptr(loss),
                                      lib.ptr(ga), lib.ptr(gb), s), "pair_loss")
    out = dict(loss=loss)
    if ga is not None:
        out["ga"] = ga
    if gb is not None:
        out["gb"] = gb
    return out


def run_pair_batch(i):
    lib, L, s = _L()
    jobs = i["jobs"]
    arr = (lib.EsrPairJob * len(jobs))()
    keep, out = [], {}
    loss = _d(i["loss0"].reshape(1)).clone()
    p = lambda t: None if t is None else t.data_ptr()
    for k, (jb, job) in enumerate(zip(arr, jobs)):
        a, b, m, c, ga, gb = dev = _pair_dev(job)
        keep.append(dev)
        jb.a, jb.b, jb.rows, jb.cols, jb.row_mask, jb.mask_value = p(a), p(b), a.shape[0], a.shape[1], p(m), job["mask_value"]
        jb.count_dev, jb.kind, jb.w_value, jb.w_a, jb.w_b, jb.ga, jb.gb = p(c), job["kind"], job["w_value"], job["w_a"], job["w_b"], \
            p(ga), p(gb)
        if ga is not None:
            out[f"job{k}_ga"] = ga
        if gb is not None:
            out[f"job{k}_gb"] = gb
    lib.check(L.esr_pair_loss_batch(arr, len(jobs), lib.ptr(loss), s), "pair_loss_batch")
    torch.cuda.synchronize()
    out["loss"] = loss
    return out


def run_coarse_shade_fwd(i):
    lib, L, s = _L()
    keep = [_d(i[k]) for k in ("z_off", "z_emo", "rec_ray", "rec_w")]
    rgb, srgb = torch.full((i["tiles_all"], 4, 32), 9.0, device=DEV), _d(i["srgb0"]).clone()
    lib.check(L.esr_coarse_shade_fwd(*[lib.ptr(t) for t in keep], i["tiles_on"], i["tiles_all"], lib.ptr(rgb), lib.ptr(srgb), s),
              "coarse_shade_fwd")
    return dict(rgb=rgb, srgb_marched=srgb)


def run_coarse_shade_bwd(i):
    lib, L, s = _L()
    keep = [_d(i[k]) for k in ("g_srgb", "g_wbg", "rgb", "z_off", "z_emo", "rec_ray", "rec_w")]
    T = i["tiles_all"]
    dz_off, dz_emo, dw = torch.full((T, 4, 32), 9.0, device=DEV), _d(i["dz_emo0"]).clone(), torch.full((T * 32,), 9.0, device=DEV)
    lib.check(L.esr_coarse_shade_bwd(*[lib.ptr(t) for t in keep], i["tiles_on"], T, lib.ptr(dz_off), lib.ptr(dz_emo), lib.ptr(dw), s),
              "coarse_shade_bwd")
    return dict(dz_off=dz_off, dz_emo=dz_emo, dweight=dw)


def run_eval_aux(i):
    lib, L, s = _L()
    X, rr, st = _d(i["X"]), _d(i["rec_ray"]), _d(i["rec_step"])
    T = i["tiles_all"]
    aux = torch.full((T, 8, 32), 9.0, device=DEV)
    rt = (C.c_float * 9)(*i["rt"])
    lib.check(L.esr_eval_aux(lib.ptr(X), X.shape[1], *i["nrow"], lib.ptr(rr), lib.ptr(st), T, rt, _f(i["stepdist"]), lib.ptr(aux), s),
              "eval_aux")
    return dict(aux=aux)


def run_eval_disp(i):
    lib, L, s = _L()
    d3, al = _d(i["depth3"]), _d(i["last"])
    n = i["n_rays"]
    depth, disp = torch.full((n,), 9.0, device=DEV), torch.full((n,), 9.0, device=DEV)
    lib.check(L.esr_eval_disp(lib.ptr(d3), lib.ptr(al), _f(i["far"]), n, lib.ptr(depth), lib.ptr(disp), s), "eval_disp")
    return dict(depth=depth, disp=disp)


RUN = {"tone_in_fwd": run_tone_in_fwd, "tone_in_bwd": run_tone_in_bwd, "lts_tone_in_bwd": run_lts_tone_in_bwd,
       "composite_fwd": run_composite_fwd, "composite_bwd": run_composite_bwd, "loss": run_loss,
       "composite3_fwd": run_composite3_fwd, "composite3_bwd": run_composite3_bwd, "act": run_act, "act_batch": run_act_batch,
       "pair_loss": run_pair_loss, "pair_batch": run_pair_batch, "coarse_shade_fwd": run_coarse_shade_fwd,
       "coarse_shade_bwd": run_coarse_shade_bwd, "eval_aux": run_eval_aux, "eval_disp": run_eval_disp}


@pytest.mark.parametrize("op,case", R.all_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_kernel_against_the_float64_restatement(op, case):
    assert set(RUN) == set(R.OPS)
    inp = R.build(op, case)
    got = {k: v.cpu() for k, v in RUN[op](inp).items()}
    fam = R.OPS[op][4]
    ref, worst, fails = R.verify(op, inp, got, K_FAMILY[fam])
    WORST[fam] = max(WORST.get(fam, 0.0), worst)
    census = set(inp.get("census", ()))
    if op == "loss":
        census = R.loss_census(inp, ref)
        for k, n in ref.flips.items():
            FLIPS[k] = FLIPS.get(k, 0) + n
    CENSUS.setdefault(fam, set()).update(census)
    print(f"\n[{op} {case}] worst |gpu - ref| / (U absref) = {worst:.3g} (K = {K_FAMILY[fam]}); flips {ref.flips} "
          f"({ref.share:.4%}); census: {sorted(census)}")
    assert not fails, fails
    assert ref.share <= R.FLIP_CAP, f"{ref.share:.3%} of the values exempted as decision flips"
    if "claims" in inp:
        assert inp["claims"] <= census, inp["claims"] - census


TILE_CLASSES = {"tiles_all=1", "tiles_all=2", "tiles_all odd", "tiles_all even", "tiles_on=0", "tiles_on odd", "tiles_on even",
                "tiles_on=tiles_all", "on-group ends mid-tile", "second grid-stride trip", "0 survivors", "1 survivor", "32 survivors",
                "64 survivors", "more than 64 survivors", "several atomics per ray", "ray ends in lane 0", "ray ends in lane 31",
                "ray ends in lane 63", "all-padding tile", "z == 20", "z just above 20", "z just below 20", "z = 30", "z = -30",
                "z = -100", "16 lin of tens of radians", "gradient scale 1", "gradient scale 0.0001", "gradient scale 1e-07",
                "weights 0 and 1", "non-zero accumulators"}
LOSS_CLASSES = {"ps inside", "not ps inside", "pl >= 0", "not pl >= 0", "x below the knee", "not x below the knee",
                "gt >= 1, l0 <= 1", "gt >= 1, l0 > 1", "last ray inside", "last ray below", "last ray above", "last ray at_lo",
                "last ray at_hi", "exact boundaries", "d == 0"}


def test_the_cases_reach_every_class():
    """the union of the cases' own censuses (computed on the CPU from the shared inputs) covers the issue's classes"""
    tile = set()
    for name in R.TILE_CASES:
        tile |= R.tile_base(name)["census"]
    assert TILE_CLASSES <= tile, TILE_CLASSES - tile
    loss = set()
    for name in R.LOSS_CASES:
        inp = R.case_loss(name)
        loss |= R.loss_census(inp, R.ref_loss(inp))
    assert LOSS_CLASSES <= loss, LOSS_CLASSES - loss
    assert {c[0] for c in R.LOSS_CASES.values()} >= {1, 63, 64, 65, 777}
    assert {c[1] for c in R.LOSS_CASES.values()} == {0.0, 1.0} and {c[2] for c in R.LOSS_CASES.values()} == {1.0, 0.25}
    assert "d == 0" in R.pair_jobs()["l1"]["census"]                       # sign(0) = 0
    assert len(R.case_pair_batch("full")["jobs"]) == R.PAIR_MAX_JOBS and len(R.case_act_batch("full")["jobs"]) == R.ACT_MAX_JOBS
    print("\nworst ratio per family:", {k: round(v, 3) for k, v in sorted(WORST.items())})
    print("decision flips:", FLIPS)
    for fam, c in sorted(CENSUS.items()):
        print(f"census[{fam}]:", sorted(c))
