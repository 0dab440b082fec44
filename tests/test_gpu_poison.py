"""No result depends on uninitialised device memory: every scenario runs three legs (tests/poison.py: A zeros, B quiet NaN,
C 2^100 / int 1), each from a fresh model built with the same seeds, with ``poisoned_allocations`` spanning the model's
construction and the whole run and ``repoison`` before every step; the poisoned legs must give what the twin gives.

Float outputs are held to the bar the project already uses for two runs of the same step (the order of float atomics
differs from run to run): rel_err < 1e-5 for the fine and coarse steps (test_gpu_train_loop.py:163), < 2e-5 for the LTS
steps (test_gpu_lts_path.py:312).  ``DETERMINISTIC_*`` list the outputs that must be bit-identical, each with the reason.
Every scenario prints its byte counts, the stale tiles / lanes it had and the worst rel_err between legs."""
import warnings

import numpy as np
import pytest
import torch

import poison
from poison import BAR_FINE, BAR_LTS, LEGS, compare, poisoned_allocations, repoison

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LRS = dict(off_color=0.1, off_rgbnet=0.003, emo_color=0.1, emo_rgbnet=0.003, sdf=0.005, tonemapper=0.003)
TVS = dict(sdf=0.1, smooth_grad=0.05)

# Bit-identical across legs.  "no atomic": no float atomic on the output's path.
DETERMINISTIC_FINE = (
    "render/last",      # alphainv_last: one wave per ray, serial transmittance scan (csrc/march.hip: march_kernel), no atomic
)
DETERMINISTIC_COARSE = ("out/etc/alphainv_cum",)        # as render/last (the same march kernel)
DETERMINISTIC_LTS = ()                                  # every output of the LTS steps sits behind a float-atomic segment sum


def _clone(x):
    if torch.is_tensor(x):
        return x.detach().clone()
    if isinstance(x, dict):
        return {k: _clone(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_clone(v) for v in x]
    return x


def _tiles(counts):
    return (counts["n_on"] + 31) // 32 + (counts["n_off"] + 31) // 32


class _Log:
    """What a leg saw: per step the samples, tiles and capacity; the bytes poisoned by the hook and by the walker."""

    def __init__(self):
        self.steps, self.repoisoned, self.pa = [], 0, None

    def step(self, counts, cap):
        self.steps.append(dict(samples=counts.get("m3", 0), tiles=_tiles(counts) if "n_on" in counts else 0, cap=cap))

    def assert_not_vacuous(self):
        assert any(s["samples"] % 32 for s in self.steps), self.steps                      # stale lanes in a last tile
        assert any(0 < s["tiles"] < s["cap"] for s in self.steps), self.steps              # stale tiles behind the last one
        assert self.pa.allocations > 0 and self.pa.bytes > 0 and self.repoisoned > 0

    def line(self):
        most = 0
        stale_tiles = []
        for s in self.steps:
            stale_tiles.append(max(most, s["cap"]) - s["tiles"] if s["cap"] else 0)
            most = max(most, s["tiles"])
        lanes = [(-s["samples"]) % 32 for s in self.steps]
        return (f"allocations {self.pa.allocations}, {self.pa.bytes} B poisoned at allocation, {self.repoisoned} B re-poisoned; "
                f"stale tiles per step {stale_tiles}, stale lanes in the ragged tiles {lanes} (samples {[s['samples'] for s in self.steps]})")


def _check(name, legs, deterministic, bar):
    """legs: {leg: (list of per-step result dicts, _Log)} -> compares B and C with A, prints the scenario's line."""
    (ra, la) = legs["A"]
    worst = worst_p = 0.0
    for leg in ("B", "C"):
        rb, lb = legs[leg]
        assert len(ra) == len(rb)
        for i, (a, b) in enumerate(zip(ra, rb)):
            if "params" in a:
                a, b = dict(a), dict(b)
                worst_p = max(worst_p, _compare_params(name, leg, i, a.pop("params"), b.pop("params")))
            try:
                errs = compare(a, b, deterministic=deterministic, bar=bar)
            except poison.Mismatch as e:
                raise AssertionError(f"{name}: leg {leg}, step {i}: {e}") from None
            worst = max([worst] + list(errs.values()))
        lb.assert_not_vacuous()
    la.assert_not_vacuous()
    print(f"\npoison[{name}]: {legs['B'][1].line()}; worst rel_err between legs {worst:.2e} (bar {bar:g})"
          + (f"; parameters after one Adam step at most {worst_p:.2e} of their max-norm apart" if worst_p else ""))


def _three_legs(run):
    """run(leg, twin) -> (results, log): leg A first, its results handed to B and C."""
    legs = {"A": run("A", None)}
    for leg in ("B", "C"):
        legs[leg] = run(leg, legs["A"][0])
    return legs


# ---- a. the fine trainer ---------------------------------------------------------------------------------------------------
def _fine_model(dtype):
    from esr_nerf_amd.config import fine_cfg
    from esr_nerf_amd.synthetic import init_slab_model, slab_scene
    from esr_nerf_amd.voxurff import VoxurfF
    sc = slab_scene("g16", s_val=40.0, oblique=True, n_rays=512, seed=3)
    torch.manual_seed(0)
    np.random.seed(0)
    m = VoxurfF(fine_cfg(DEV), sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max, sc.mask_alpha_init,
                sc.mask_density, sc.s_val, sc.num_voxels)
    m.mlp_dtype = dtype                                    # read when the engine is created (VoxurfF.engine)
    init_slab_model(m, sc)
    m.set_nonempty_mask()
    m.train()
    return m, sc


def _fine_batches(sc):
    b = {k: v.to(DEV) for k, v in sc.batch.items()}
    few = {k: v[:37].contiguous() for k, v in b.items()}
    miss = dict(b, rays_o=b["rays_o"] + torch.tensor([10.0, 0.0, 0.0], device=DEV))       # no ray enters the box
    return [b, few, miss, b, few]


def _spy_on_render(eng, sink, after=None):
    """The step's render outputs are handed to ``loss_fwd_bwd`` between the forward and the backward: note them there."""
    orig = eng.loss_fwd_bwd

    def spy(last, srgb, lin, *args, **kw):
        sink.update(last=last, srgb=srgb, lin=lin)
        out = orig(last, srgb, lin, *args, **kw)
        if after is not None:
            after()
        return out
    eng.loss_fwd_bwd = spy


def _opt_state(m, opt):
    out = {}
    for n, p in m.named_parameters():
        st = opt.state.get(p)
        if st:
            out[n] = dict(exp_avg=st["exp_avg"].detach().clone(), exp_avg_sq=st["exp_avg_sq"].detach().clone(), step=int(st["step"]))
    return out


def _adopt_state(m, opt, res):
    """Continue from the twin's parameters and moments (copied in place: same tensors, same addresses)."""
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(res["params"][n])
            st = opt.state.get(p)
            if st:
                st["exp_avg"].copy_(res["moments"][n]["exp_avg"])
                st["exp_avg_sq"].copy_(res["moments"][n]["exp_avg_sq"])


def _compare_params(name, leg, i, a, b):
    """Parameters after ONE Adam step from the same state.  Adam turns the float atomics' run-to-run noise in a gradient that
    is ~ 0 into lr * sign(noise), so two runs of the same step are not within 1e-5 of each other here; the bar is the one
    the project already holds two runs to after Adam steps (test_gpu_train_loop.py:87-96, with its 6 steps -> 1): all but
    a vanishing share of every tensor within 1e-2 of its max-norm, and no element further apart than Adam can carry it in
    one step (2 lr).  Gradients and both moments -- linear / quadratic in the gradient -- are held to the 1e-5 bar."""
    worst = 0.0
    for k, v in a.items():
        w = b[k]
        assert bool(torch.isfinite(w).all()), f"{name}: leg {leg}, step {i}: params/{k} not finite"
        lr = next((r for n_, r in LRS.items() if k.startswith(n_)), None)
        if lr is None:                                                   # not trained (the TV term's fixed convolution): untouched
            assert torch.equal(w, v), f"{name}: leg {leg}, step {i}: params/{k}"
            continue
        d = (w.double() - v.double()).abs()
        scale = float(v.double().abs().max().clamp_min(1e-12))
        assert float((d > 1e-2 * scale).double().mean()) < 1e-3, f"{name}: leg {leg}, step {i}: params/{k}"
        assert float(d.max()) <= 2 * lr * 1.05, f"{name}: leg {leg}, step {i}: params/{k} moved {float(d.max())} > 2 lr"
        worst = max(worst, float(d.max()) / scale)
    return worst


def _fine_leg(leg, dtype="f32", live=False, plant=None, twin=None):
    """Five steps of FineStep + Adam: 512 rays, 37 rays, an all-miss batch, 512 rays, 37 rays; steps 1 and 4 with the TV lines.
    ``plant``: (step index, callable(engine)) run between that step's forward and its backward (the teeth test).
    ``twin``: the results of leg A -- after every step the leg continues from the twin's parameters and moments, so that
    every step is compared on identical inputs (the atomics' noise, amplified by Adam, would otherwise compound over the
    five steps: two unpoisoned runs drift 4e-5 apart in sdf.grid).  Poison lives in scratch, never in what is adopted."""
    from esr_nerf_amd.optimizer import create_optimizer_or_freeze_model
    from esr_nerf_amd.trainer import FineStep
    fpat, ival = LEGS[leg]
    log, results = _Log(), []
    with poisoned_allocations(fpat, ival) as pa:
        log.pa = pa
        m, sc = _fine_model(dtype)
        opt = create_optimizer_or_freeze_model(m, live_bricks=live, **LRS)
        step = FineStep(m)
        if live:
            opt.zero_grads = True
            step.zero_fill_by = opt
        eng = m.engine
        if eng.range_flag is not None:
            eng.range_flag.zero_()
        sink, now = {}, [0]
        _spy_on_render(eng, sink, after=(lambda: plant[1](eng) if now[0] == plant[0] else None) if plant else None)
        for i, batch in enumerate(_fine_batches(sc)):
            now[0] = i
            rep = repoison([step, opt], fpat, ival)
            log.repoisoned += rep.bytes
            assert i == 0 or any(path.endswith("._flat") for path, _ in rep.names)      # param.grad views do not shield it
            reg = dict(n_rays_global=batch["rgbs"].shape[0], weight_tv_density=0.01, tvs=TVS, dense_mode=True) if i in (0, 3) else None
            loss, grads = step.forward_loss_backward(batch, 40.0, regularisers=reg)
            torch.cuda.synchronize()
            res = dict(loss=_clone(loss), grads=_clone(grads), render=_clone(sink), counts=dict(m.last_counts),
                       fallbacks=eng.split_fallback_steps, calls=eng.n_calls)
            log.step(m.last_counts, eng.ws.cap_tiles)
            step.assign_grads(grads)
            opt.step()
            torch.cuda.synchronize()
            res["params"] = {n: p.detach().clone() for n, p in m.named_parameters()}
            res["moments"] = _opt_state(m, opt)
            if live:
                res["live"] = opt.live_stats()
                res["flat_grid_nonzero"] = int(torch.count_nonzero(step._flat[:step._n_grid]))
            results.append(res)
            if plant and i == plant[0]:
                break
            if twin is not None:
                _adopt_state(m, opt, twin[i])
    assert eng.bf16 == (dtype == "bf16")
    return results, log


@pytest.mark.parametrize("engine", ["split", "f32_mfma", "bf16"])
def test_fine_trainer_steps_do_not_depend_on_stale_memory(engine, monkeypatch):
    if engine == "f32_mfma":
        monkeypatch.setenv("ESR_SPLIT_FWD", "0")          # read in FineEngine.__init__
    else:
        monkeypatch.delenv("ESR_SPLIT_FWD", raising=False)
    legs = _three_legs(lambda leg, twin: _fine_leg(leg, dtype="bf16" if engine == "bf16" else "f32", twin=twin))
    assert legs["A"][0][2]["counts"]["m3"] == 0 and legs["A"][0][0]["counts"]["m3"] > legs["A"][0][1]["counts"]["m3"] > 64
    _check(f"fine/{engine}", legs, DETERMINISTIC_FINE, BAR_FINE)


def test_fine_trainer_with_the_live_brick_optimizer_deciding_the_zero_fill(monkeypatch):
    from esr_nerf_amd import optimizer
    monkeypatch.delenv("ESR_SPLIT_FWD", raising=False)
    monkeypatch.setattr(optimizer, "LIVE_MIN_NUMEL", 512)            # the g16 grids count as large (test_gpu_adam_live.py)
    legs = _three_legs(lambda leg, twin: _fine_leg(leg, live=True, twin=twin))
    for res, _ in legs.values():
        assert all(set(r["live"]) >= {"sdf", "off_color", "emo_color"} for r in res), res[0]["live"]
        assert all(r["flat_grid_nonzero"] == 0 for r in res)         # the live kernel's fill
    _check("fine/split+live-brick Adam", legs, DETERMINISTIC_FINE, BAR_FINE)


# ---- g. teeth on the device ------------------------------------------------------------------------------------------------
def test_poison_in_a_buffer_that_is_read_reaches_the_comparison(monkeypatch):
    """Step 2 (37 rays) of the fine scenario with one LIVE buffer treated as scratch: ``ws["H0"]`` -- the first hidden
    activations, which the weight gradients read -- is poisoned between the forward and the backward of the same step."""
    monkeypatch.delenv("ESR_SPLIT_FWD", raising=False)
    twin, _ = _fine_leg("A", plant=(1, lambda eng: None))
    bad, _ = _fine_leg("A", plant=(1, lambda eng: poison.fill(eng.ws["H0"], poison.NAN, 0)), twin=twin)
    rest = lambda r: {k: v for k, v in r.items() if k != "params"}      # (parameters after Adam: _compare_params' bar)
    compare(rest(twin[0]), rest(bad[0]), DETERMINISTIC_FINE, BAR_FINE)   # the step before it: untouched
    _compare_params("teeth", "A", 0, twin[0]["params"], bad[0]["params"])
    with pytest.raises(poison.Mismatch, match="non-finite"):
        compare(rest(twin[1]), rest(bad[1]), DETERMINISTIC_FINE, BAR_FINE)
    g = bad[1]["grads"]
    hit = [k for k, v in g.items() if not bool(torch.isfinite(v).all())]
    assert hit and all("rgbnet" in k and k.endswith("weight") for k in hit), hit      # the weight gradients dZ1 x H0, nothing else
    assert bool(torch.isfinite(g["sdf.grid"]).all()) and bool(torch.isfinite(g["tonemapper.srgb.0.weight"]).all())


# ---- b. the range fallback -------------------------------------------------------------------------------------------------
def _heal_leg(leg):
    """The recipe of test_gpu_split.py::test_trainer_step_heals_a_hidden_activation_overflow_in_the_same_step: a normal
    step, the healed step (a first-layer bias of 7e4 in the emo net), then -- with NO re-poisoning: the abandoned split pass
    is the project's own source of Inf in the workspace -- a normal step, then one more with re-poisoning."""
    from esr_nerf_amd.synthetic import slab_scene
    from esr_nerf_amd.trainer import FineStep
    from test_gpu_fine_path import build_gpu_model, gpu_batch
    fpat, ival = LEGS[leg]
    log, results = _Log(), []
    with poisoned_allocations(fpat, ival) as pa:
        log.pa = pa
        sc = slab_scene("small", s_val=60.0, oblique=True, n_rays=384, seed=9, mask="prune")
        b = gpu_batch(sc)
        m = build_gpu_model(sc, seed=1, grid_seed=2)
        eng = m.engine
        assert eng.split_fwd
        eng.range_flag.zero_()
        step = FineStep(m)
        lin = m.emo_rgbnet.layers()[0]
        keep = lin.bias.data.clone()
        for i in range(4):
            if i != 2:
                log.repoisoned += repoison(step, fpat, ival).bytes
            if i == 1:
                lin.bias.data[3] = 7.0e4
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                loss, grads = step.forward_loss_backward(b, 60.0)
            torch.cuda.synchronize()
            if i == 1:
                lin.bias.data.copy_(keep)
            results.append(dict(loss=_clone(loss), grads=_clone(grads), counts=dict(m.last_counts),
                                fallbacks=eng.split_fallback_steps, flag=int(eng.range_flag), split=bool(eng.split_fwd)))
            log.step(m.last_counts, eng.ws.cap_tiles)
        step.close()
    return results, log


def test_range_fallback_heals_on_poisoned_workspaces(monkeypatch):
    monkeypatch.delenv("ESR_SPLIT_FWD", raising=False)
    legs = {leg: _heal_leg(leg) for leg in LEGS}
    assert [r["fallbacks"] for r in legs["A"][0]] == [0, 1, 1, 1] and all(r["flag"] == 0 and r["split"] for r in legs["A"][0])
    _check("range fallback", legs, (), BAR_FINE)


# ---- c. LTS / PDRA / fine-tune ---------------------------------------------------------------------------------------------
N_LTS, N_LTS_FEW = 256, 101


def _lts_leg(leg, kind):
    """``kind``: "lts" / "pdra" (LtsStep) or "finetune" (FinetuneStep): one step at 256 rays, one at 101, num_ltspts = 23."""
    from esr_nerf_amd.config import lts_cfg
    from esr_nerf_amd.esrnerf import ESRNeRF
    from esr_nerf_amd.synthetic import init_slab_model, slab_scene
    from esr_nerf_amd.trainer import FinetuneStep, LtsStep
    fpat, ival = LEGS[leg]
    log, results = _Log(), []
    s_val = 60.0
    with poisoned_allocations(fpat, ival) as pa:
        log.pa = pa
        sc = slab_scene("g16", s_val=s_val, oblique=True, n_rays=N_LTS, seed=2)
        torch.manual_seed(0)
        np.random.seed(0)
        cfg = lts_cfg(DEV, num_2ndrays=8, num_ltspts=23)
        m = ESRNeRF(cfg, sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max, sc.mask_alpha_init,
                    sc.mask_density, sc.s_val, sc.num_voxels)
        init_slab_model(m, sc, seed=3)
        with torch.no_grad():
            m.brdf.grid.normal_(0.0, 0.3, generator=torch.Generator(device=DEV).manual_seed(6))
        m.train()
        b = {k: v.to(DEV) for k, v in sc.batch.items()}
        b["uncert_masks"] = (torch.arange(N_LTS, device=DEV) % 3 == 0)
        if kind == "finetune":
            m.train(True, finetune=True)
            b.update(em_intensities=torch.ones(N_LTS, device=DEV), em_colors=torch.full((N_LTS, 2), 0.5, device=DEV))
            step = FinetuneStep(m)
        else:
            m.pdra_mode = kind == "pdra"
            step = LtsStep(m, cfg.app.trainer, stage=kind)
        eng = m.engine
        if eng.range_flag is not None:
            eng.range_flag.zero_()
        torch.manual_seed(11)                                 # the step's own draws: the same in every leg
        np.random.seed(11)
        for n in (N_LTS, N_LTS_FEW):
            batch = {k: v[:n].contiguous() for k, v in b.items()}
            log.repoisoned += repoison(step, fpat, ival).bytes
            out = step.forward_loss_backward(batch, s_val)
            torch.cuda.synchronize()
            res = dict(loss=_clone(out[0]), grads=_clone(out[1]), counts=dict(m.last_counts), fallbacks=eng.split_fallback_steps,
                       passes={p.name: (p.tiles_on, p.tiles_all) for p in (eng.prim, eng.pts, eng.sec, eng.epsp)})
            if len(out) > 2:
                res["out"] = _clone(out[2])
            results.append(res)
            log.step(m.last_counts, eng.prim.cap)
    return results, log


@pytest.mark.parametrize("kind", ["lts", "pdra", "finetune"])
def test_lts_steps_do_not_depend_on_stale_memory(kind, monkeypatch):
    monkeypatch.delenv("ESR_SPLIT_FWD", raising=False)
    legs = {leg: _lts_leg(leg, kind) for leg in LEGS}
    _check(f"lts/{kind}", legs, DETERMINISTIC_LTS, BAR_LTS)


# ---- d. coarse and pre-stage -----------------------------------------------------------------------------------------------
def _coarse_leg(leg):
    """VoxurfC through its autograd route (the coarse trainer's): one training step at 512 rays, one at 37."""
    from esr_nerf_amd.synthetic import slab_scene
    from oracle import coarse_path as cp
    from test_gpu_coarse import build_coarse_model
    fpat, ival = LEGS[leg]
    log, results = _Log(), []
    with poisoned_allocations(fpat, ival) as pa:
        log.pa = pa
        sc = slab_scene("g16", s_val=8.0, oblique=True, n_rays=512, seed=4)
        m, cfg = build_coarse_model(sc)
        b = {k: v.to(DEV) for k, v in sc.batch.items()}
        for n in (512, 37):
            bb = {k: v[:n].contiguous() for k, v in b.items()}
            log.repoisoned += repoison(m, fpat, ival).bytes
            m.zero_grad(set_to_none=True)
            res = m(rays_o=bb["rays_o"], rays_d=bb["rays_d"], viewdirs=bb["viewdirs"], em_modes=bb["em_modes"], s_val=8.0)
            loss, _ = cp.coarse_loss(res, bb["rgbs"], True, cfg.app.trainer.weight_entropy_last)
            loss.backward()
            torch.cuda.synchronize()
            results.append(dict(loss=_clone(loss), out=_clone(dict(res)), counts=dict(m.last_counts),
                                grads={k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}))
            log.step(m.last_counts, m.engine.ws.cap_tiles)
    return results, log


def test_coarse_steps_do_not_depend_on_stale_memory():
    legs = {leg: _coarse_leg(leg) for leg in LEGS}
    assert len(legs["A"][0][0]["grads"]) == 15
    _check("coarse", legs, DETERMINISTIC_COARSE, BAR_FINE)


def _dvgo_leg(leg):
    """DVGO on its smallest existing case (tests/golden/dvgo_small.npz): training with the golden's upstream gradients,
    evaluation in both modes, the view count."""
    from test_gpu_dvgo import FOUR, GRIDS, golden_case
    fpat, ival = LEGS[leg]
    with poisoned_allocations(fpat, ival) as pa:
        z, m, b = golden_case()
        res = m.render_training(b["rays_o"], b["rays_d"], b["em_modes"], b["jitter"])
        up = {k: torch.from_numpy(z["up/" + k]).to(DEV) for k in FOUR}
        gs = torch.autograd.grad(sum((res[k] * up[k]).sum() for k in FOUR), [getattr(m, k) for k in GRIDS])
        out = dict(train=_clone(dict(res)), grads={k: g.clone() for k, g in zip(GRIDS, gs)})
        assert repoison(m, fpat, ival).filled == 0              # the pre-stage keeps no workspace: everything it holds is STATE
        with torch.no_grad():
            for mode in (0, 1):
                out[f"eval{mode}"] = _clone(dict(m.eval()(rays_o=b["rays_o"], rays_d=b["rays_d"], em_modes=mode)))
        m.train()
        vo, vd = torch.from_numpy(z["views_o"]).to(DEV), torch.from_numpy(z["views_d"]).to(DEV)
        out["count"] = m.voxel_count_views(vo, vd, 50).clone()
        torch.cuda.synchronize()
    return out, pa


# DVGO: the forward gathers and composites per ray in one thread each (csrc/dvgo.hip), no atomic: every training and evaluation
# output and the view count (integer-valued sums of 0 / 1) are bit-identical; the grid gradients are scattered with float atomics
DETERMINISTIC_DVGO = ("train", "eval0", "eval1", "count")


def test_dvgo_does_not_depend_on_stale_memory():
    legs = {leg: _dvgo_leg(leg) for leg in LEGS}
    worst = 0.0
    for leg in ("B", "C"):
        worst = max([worst] + list(compare(legs["A"][0], legs[leg][0], DETERMINISTIC_DVGO, BAR_FINE).values()))
        assert legs[leg][1].bytes > 0
    pa = legs["B"][1]
    print(f"\npoison[dvgo]: allocations {pa.allocations}, {pa.bytes} B poisoned at allocation (no kept workspace: nothing to re-poison); "
          f"worst rel_err between legs {worst:.2e} (bar {BAR_FINE:g})")


# ---- e. evaluation ---------------------------------------------------------------------------------------------------------
H, W, BATCH = 33, 31, 300                        # 1023 rays: three full chunks and a ragged one of 123 (LPIPS needs 31 x 31)


def _eval_leg(leg):
    """One training step, then ``render_view`` on the same engine (a batch size that leaves a ragged last chunk),
    ``postprocess_view`` and ``view_metrics`` with the LPIPS term."""
    from esr_nerf_amd.evaluate import postprocess_view, render_view, view_metrics
    from esr_nerf_amd.lpips import LpipsAlex
    from esr_nerf_amd.synthetic import slab_scene
    from esr_nerf_amd.trainer import FineStep
    fpat, ival = LEGS[leg]
    log = _Log()
    with poisoned_allocations(fpat, ival) as pa:
        log.pa = pa
        m, sc = _fine_model("f32")
        step = FineStep(m)
        eng = m.engine
        eng.range_flag.zero_()
        log.repoisoned += repoison(step, fpat, ival).bytes
        step.forward_loss_backward({k: v.to(DEV) for k, v in sc.batch.items()}, 40.0)
        log.step(m.last_counts, eng.ws.cap_tiles)
        view = slab_scene("g16", s_val=40.0, oblique=True, n_rays=H * W, seed=8)
        rays = {k: view.batch[k].to(DEV) for k in ("rays_o", "rays_d", "viewdirs")}
        g = torch.Generator().manual_seed(1)
        rgbs, hdrs = torch.rand(H, W, 3, generator=g).to(DEV), (torch.rand(H, W, 3, generator=g) * 1.5).to(DEV)
        log.repoisoned += repoison(step, fpat, ival).bytes
        m.eval()
        raw = render_view(m, rays["rays_o"], rays["rays_d"], rays["viewdirs"], 1, torch.eye(3, device=DEV), H, W, BATCH)
        tiles = eng.last_eval_counts["tiles"]                  # (of the last, ragged chunk)
        log.steps.append(dict(samples=int((eng.ws["rec_ray"][: tiles * 32] >= 0).sum()), tiles=tiles, cap=eng.ws.cap_tiles))
        post = postprocess_view(raw, True, rgbs=rgbs, hdrs=hdrs, want_u8=True)
        metrics = view_metrics(post, rgbs, hdrs=hdrs, em_mode=1, lpips=LpipsAlex.random(0, DEV))
        torch.cuda.synchronize()
        out = dict(raw=_clone(raw), post=_clone(dict(post)), u8=_clone(post.u8), sqerr=_clone(post.sqerr),
                   metrics={k: v for k, v in metrics.items() if v is not None}, fallbacks=eng.split_fallback_steps)
    return [out], log


# Evaluation: every image is a per-ray segment sum with one float atomic per (ray, wave) (csrc/shade.hip: composite_fwd,
# composite3_fwd).  At g16's 16 samples a ray's records touch at most two waves, and a sum of at most two floats onto +0 does
# not depend on their order: bit-identical.  Post-processing, the error sums (float64, fixed order), SSIM and LPIPS (no
# atomics: csrc/metrics.hip, csrc/lpips.hip) are functions of the images.
DETERMINISTIC_EVAL = ("raw", "post", "u8", "sqerr", "metrics")


def test_evaluation_after_a_training_step_does_not_depend_on_stale_memory(monkeypatch):
    monkeypatch.delenv("ESR_SPLIT_FWD", raising=False)
    legs = {leg: _eval_leg(leg) for leg in LEGS}
    assert {"srgb/PSNR", "srgb/SSIM", "lin/PSNR", "lin/SSIM", "lin/LPIPS_ALEX", "srgb/LPIPS_ALEX"} <= set(legs["A"][0][0]["metrics"])
    _check("evaluation", legs, DETERMINISTIC_EVAL, BAR_FINE)


# ---- f. Python wrappers with their own scratch and outputs ------------------------------------------------------------------
# One smallest existing case each; every output must be torch.equal across the legs.  Before a wrapper was added here, the
# kernels behind it were read for index safety (tests/poison.py): its integer scratch only ever holds 0 / 1, and no float
# buffer it allocates becomes an address.  Left out, for the next pull request: mesh.simplify, raycast, raster, atlas,
# sources (source_lights, environment_light, path_light), chamfer, regroup.partition (its output sizes come from a scratch
# word: a latent bug there would be a wild write, not a wrong number).
def _wrapper_legs(name, run):
    outs = {}
    for leg, (fpat, ival) in LEGS.items():
        with poisoned_allocations(fpat, ival) as pa:
            outs[leg] = _clone(run())
            torch.cuda.synchronize()
        assert pa.allocations > 0 and pa.bytes > 0, name
        outs[leg + "/pa"] = pa
    for leg in ("B", "C"):
        try:
            compare(outs["A"], outs[leg], deterministic=tuple(outs["A"]))
        except poison.Mismatch as e:
            raise AssertionError(f"{name}: leg {leg}: {e}") from None
    pa = outs["B/pa"]
    print(f"\npoison[{name}]: allocations {pa.allocations}, {pa.bytes} B poisoned at allocation; every output bit-identical")


def test_mesh_field_marching_cubes_and_components():
    from esr_nerf_amd.mesh import connected_components, marching_cubes, sdf_field
    from test_gpu_mesh import _fine_model, _sphere_grid

    def run():
        m = _sphere_grid(_fine_model("g16"))
        u = sdf_field(m, 37)
        v, f = marching_cubes(u, 0.0)
        label, k = connected_components(f, v.shape[0])
        assert v.shape[0] > 100 and f.shape[0] > 100 and k >= 1
        return dict(field=u, vertices=v, triangles=f, label=label, k=k)
    _wrapper_legs("mesh", run)


def test_grid_setup_resample_pool_mask_and_bounds():
    from esr_nerf_amd import gridsetup

    def run():
        g = torch.Generator().manual_seed(3)
        vol = torch.randn(13, 9, 7, 6, generator=g).to(DEV)
        dens = (torch.randn(1, 1, 21, 17, 11, generator=g) * 4).to(DEV)
        pooled = gridsetup.maxpool3d(dens, 3)
        box = (torch.tensor([-1.0, -0.8, -0.5]), torch.tensor([0.9, 1.0, 0.6]))
        axes = gridsetup.bounds_axes(box[0].to(DEV), box[1].to(DEV), (19, 23, 5))
        sdf = torch.randn(19, 23, 5, generator=g).to(DEV)
        mask, count = gridsetup.nonempty_mask(pooled, box, -2.0, 0.3, axes, sdf=sdf)
        lo, hi = gridsetup.density_bounds(dens, box, -2.0, 0.3)
        return dict(resampled=gridsetup.resample_grid(vol, (17, 5, 12)), scalar=gridsetup.resample_grid(vol[..., 0].contiguous(), (4, 20, 7)),
                    pooled=pooled, mask=mask, count=count, sdf=sdf, lo=lo, hi=hi)
    _wrapper_legs("gridsetup", run)


def test_ray_filter():
    from esr_nerf_amd.rayfilter import filter_rays

    def run():
        m, sc = _fine_model("f32")
        b = {k: v.to(DEV) for k, v in sc.batch.items()}
        o = torch.cat([b["rays_o"][:300], b["rays_o"][300:337] + torch.tensor([10.0, 0.0, 0.0], device=DEV)])
        d = b["rays_d"][:337]
        out = {}
        for fixed in (False, True):
            keep, first = filter_rays(m, o, d, fixed, want_first_hit=True)
            assert 0 < int(keep.sum()) < 337
            out[f"keep{int(fixed)}"], out[f"first{int(fixed)}"] = keep, first
        return out
    _wrapper_legs("rayfilter", run)


def test_regroup_decide():
    import regroup_ref as R
    from esr_nerf_amd import regroup

    def run():
        e = torch.from_numpy(R.emission_case(5000, np.float32(0.40575385), 3)).to(DEV)
        flags, stats = regroup.decide(e, 0.40575385)
        rec = regroup.read_stats(stats)
        rec.pop("totals")                                  # (written by the partition's scan, not by decide)
        return dict(flags=flags, **{k: float(v) for k, v in rec.items()})
    _wrapper_legs("regroup.decide", run)


def test_relight_dilation_and_labels():
    import relight_ref
    from esr_nerf_amd.relight import dilate_masks
    from test_gpu_relight import Z, _label_case

    def run():
        rng = np.random.default_rng(11037)
        m = rng.random((3, 37, 53)).astype(np.float32)
        m[rng.random((3, 37, 53)) < 0.8] = 0.0
        out = dict(dilated=dilate_masks(torch.from_numpy(m).cuda(), 10))
        out.update({k: torch.from_numpy(v) for k, v in _label_case(relight_ref.case(Z, "tall"), return_uv=True).items()})
        return out
    _wrapper_legs("relight", run)


def test_metrics_post_image_error_sums_and_ssim():
    from esr_nerf_amd import metrics

    def run():
        g = torch.Generator().manual_seed(4)
        img = (torch.rand(37, 29, 3, generator=g) * 1.6 - 0.2).to(DEV)
        tgt = torch.rand(37, 29, 3, generator=g).to(DEV)
        wbg = torch.rand(37, 29, generator=g).to(DEV)
        r = metrics.post_image(img, wbg, 1.0, lin=True, want_u8=True, target=tgt * 1.5, target_gamma=tgt)
        return dict(post=dict(r), sqerr=metrics.sqerr_sum(img, tgt), ssim=metrics.rgb_ssim(r["gamma"], tgt, 1),
                    ssim_map=metrics.rgb_ssim(r["gamma"], tgt, 1, return_map=True))
    _wrapper_legs("metrics", run)


def test_camera_rays_and_batches():
    from conftest import load_npz
    from esr_nerf_amd.camera import Cameras, camera_batch, camera_rays
    from test_gpu_camera import _rows

    def run():
        z = load_npz("camera_rays.npz")
        cams = Cameras.from_blender(z["transform_matrices"], float(z["camera_angle_x"]), int(z["width"]), int(z["height"]), device=DEV)
        modes = torch.from_numpy(z["em_modes"].reshape(3, -1)[:, 0].copy()).to(DEV)
        rgba = torch.from_numpy(z["rgba"]).to(DEV)
        rows = _rows(cams, 200)
        out = dict(zip(("rays_o", "rays_d", "viewdirs"), camera_rays(cams, 1)))
        out["white"] = camera_batch(cams, rgba, modes, rows, True)
        out["black"] = camera_batch(cams, rgba[:, :3].contiguous(), modes, rows[:65], False)
        return out
    _wrapper_legs("camera", run)
