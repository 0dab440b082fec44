"""Live-brick Adam on the GPU (esr_adam_step_live, optimizer.Adam(live_bricks=True), _Step.zero_fill_by) against the dense
path on the same inputs: parameters and moments must be ``torch.equal`` after every step -- the mode skips only bricks on
which the update is the identity -- the flags must be the running union of the bricks that had a gradient, the fused zero
fill must leave the gradient all-zero, and the trainer step must neither skip a fill it needs nor accumulate."""
import copy
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BRICK = 128
LR, B1, B2, EPS = 0.05, 0.9, 0.99, 1e-8


def _L():
    from esr_nerf_amd import _lib
    return _lib, _lib.lib()


def _dense(p, g, m, v, plr, step, eps=EPS):
    _lib, L = _L()
    _lib.check(L.esr_adam_step(_lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), _lib.ptr(plr) if plr is not None else None,
                               C.c_int64(p.numel()), C.c_float(LR), C.c_float(B1), C.c_float(B2), C.c_float(eps),
                               C.c_float(0.0), int(step), _lib.stream_ptr(p.device)), "esr_adam_step")


def _live_rc(p, g, m, v, plr, live, step, zero, stats, eps=EPS, n=None):
    _lib, L = _L()
    return L.esr_adam_step_live(_lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), _lib.ptr(plr) if plr is not None else None,
                                _lib.ptr(live), p.numel() if n is None else n, LR, B1, B2, eps, int(step), int(zero),
                                _lib.ptr(stats) if stats is not None else None, _lib.stream_ptr(p.device))


def _brick_any(t):
    nb = -(-t.numel() // BRICK)
    pad = torch.zeros(nb * BRICK, device=t.device)
    pad[:t.numel()] = t
    return (pad.view(nb, BRICK) != 0).any(1)


def _sparse_grad(n, step, gen):
    """A random 3 % of the bricks per step (so that some stay dead for all 30), values over 1e-12 ... 50 of both signs;
    bricks with b % 7 == 3 only in step 5 (touched once); step 9 all-zero; every 13th value -0.0, in touched and
    untouched bricks alike."""
    nb = -(-n // BRICK)
    pick = torch.rand(nb, device=DEV, generator=gen) < 0.03
    once = torch.arange(nb, device=DEV) % 7 == 3
    pick = (pick & ~once) | (once & (step == 5))
    pick[nb - 1] = pick[nb - 1] | (step % 4 == 2)                 # the (ragged) last brick takes part
    mag = 10.0 ** (torch.rand(nb * BRICK, device=DEV, generator=gen) * 13.7 - 12.0)
    g = torch.randn(nb * BRICK, device=DEV, generator=gen).sign() * mag * pick.repeat_interleave(BRICK)
    if step == 9:
        g.zero_()
    g[::13] = -0.0
    return g[:n].clone()


@pytest.mark.parametrize("zero", [0, 1])
@pytest.mark.parametrize("with_plr", [False, True])
@pytest.mark.parametrize("n", [BRICK * 37, BRICK * 37 + 5, BRICK * 4096])
def test_live_kernel_equals_the_dense_kernel_step_by_step(n, with_plr, zero):
    gen = torch.Generator(device=DEV).manual_seed(n + 2 * with_plr + zero)
    nb = -(-n // BRICK)
    p = torch.randn(n, device=DEV, generator=gen)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    plr = None
    if with_plr:
        plr = torch.rand(n, device=DEV, generator=gen)
        plr[::3] = 0.0
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    live = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    union = torch.zeros(nb, dtype=torch.bool, device=DEV)
    stats = torch.zeros(2, dtype=torch.int64, device=DEV)
    p_start = p.clone()
    for step in range(1, 31):
        g = _sparse_grad(n, step, gen)
        nz = _brick_any(g)
        union |= nz
        g_live = g.clone()
        _dense(p2, g, m2, v2, plr, step)
        stats.zero_()
        assert _live_rc(p, g_live, m, v, plr, live, step, zero, stats) == 0
        assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2), step
        assert torch.equal(live.bool(), union), step
        assert stats.tolist() == [int(union.sum()), int(nz.sum())], step
        if zero:
            assert int(torch.count_nonzero(g_live)) == 0, step
        else:
            assert torch.equal(g_live, g) and torch.equal(g_live.signbit(), g.signbit()), step
    assert 0 < int(union.sum()) < nb                              # some bricks stayed dead: they were skipped, and
    dead = (~union).repeat_interleave(BRICK)[:n]
    assert torch.equal(p[dead], p_start[dead])                    # the dense kernel left them as they were


def test_live_from_moments_and_argument_errors():
    _lib, L = _L()
    n = BRICK * 9 + 3
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    m[BRICK * 2 + 5] = -1e-30
    v[BRICK * 4] = 1e-38
    v[n - 1] = 2.0                                                # in the ragged brick
    m[BRICK * 6] = -0.0
    live = torch.zeros(10, dtype=torch.uint8, device=DEV)
    live[1] = 1                                                   # |=: a set flag stays
    rc = L.esr_brick_live_from_moments(_lib.ptr(m), _lib.ptr(v), n, _lib.ptr(live), _lib.stream_ptr(m.device))
    assert rc == 0 and live.tolist() == [0, 1, 1, 0, 1, 0, 0, 0, 0, 1]
    p, g = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    assert _live_rc(p, g, m, v, None, live, 1, 0, None, eps=0.0) != 0              # eps > 0 is what the identity rests on
    assert _live_rc(p, g, m, v, None, live, 0, 0, None) != 0                       # step >= 1, as esr_adam_step
    buf = torch.zeros(n + 4, device=DEV)
    assert _live_rc(buf[1:n + 1], g, m, v, None, live, 1, 0, None) != 0            # every pointer 16-byte aligned
    assert _live_rc(p, g, m, v, None, live, 1, 0, None, n=0) == 0
    torch.cuda.synchronize()
    assert live.tolist() == [0, 1, 1, 0, 1, 0, 0, 0, 0, 1] and int(torch.count_nonzero(p)) == 0


# ---- optimizer level ---------------------------------------------------------------------------------------------------
def _params(seed=0):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    color = torch.randn(1, 6, 16, 12, 10, device=DEV, generator=gen).contiguous(memory_format=torch.channels_last_3d)
    sdf = torch.randn(1, 1, 17, 9, 5, device=DEV, generator=gen)
    w = torch.randn(192, 85, device=DEV, generator=gen)
    return [torch.nn.Parameter(t) for t in (color, sdf, w)]


def _groups(ps, **kw):
    return [dict(params=[p], lr=lr, name=n, **kw) for p, lr, n in zip(ps, (0.1, 0.005, 0.003), ("color", "sdf", "w"))]


def _grads(step, gen):
    """Shared gradients: a few z-columns of the colour grid (channels-last memory, as the trainer hands it out), a few
    cells of the sdf, a full weight gradient that arrives TRANSPOSED in memory -- which the optimizer re-stores, so the
    weight goes the dense way."""
    c = torch.zeros(1, 16, 12, 10, 6, device=DEV)
    xy = torch.rand(16, 12, device=DEV, generator=gen) < (0.0 if step == 7 else 0.02)
    c[0][xy] = torch.randn(int(xy.sum()), 10, 6, device=DEV, generator=gen)
    s = torch.zeros(1, 1, 17, 9, 5, device=DEV)
    if step % 3 == 0:
        s[0, 0, step % 17, 2:5] = torch.randn(3, 5, device=DEV, generator=gen) * 1e-4
    w = torch.randn(85, 192, device=DEV, generator=gen).t()
    return [c.permute(0, 4, 1, 2, 3), s, w]


def _set_grads(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = g.clone(memory_format=torch.preserve_format)


def _assert_same(a_ps, a_opt, b_ps, b_opt, what):
    for pa, pb in zip(a_ps, b_ps):
        assert torch.equal(pa, pb), what
    sa, sb = a_opt.state_dict()["state"], b_opt.state_dict()["state"]
    assert set(sa) == set(sb), what
    for k in sa:
        assert set(sa[k]) == set(sb[k]) == {"step", "exp_avg", "exp_avg_sq"}, what
        assert sa[k]["step"] == sb[k]["step"], what
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(sa[k][key], sb[k][key]), (what, k, key)


def test_live_optimizer_equals_the_dense_optimizer_and_exchanges_checkpoints(monkeypatch):
    from esr_nerf_amd import optimizer
    from esr_nerf_amd.optimizer import Adam
    monkeypatch.setattr(optimizer, "LIVE_MIN_NUMEL", 512)
    gen = torch.Generator(device=DEV).manual_seed(3)
    runs = {}

    def new(name, live, src=None):
        ps = _params() if src is None else [torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format)) for p in src]
        runs[name] = (ps, Adam(_groups(ps), betas=(B1, B2), live_bricks=live))
        return runs[name]

    new("dense", False)
    new("live", True)
    for step in range(1, 21):
        gs = _grads(step, gen)
        for ps, opt in runs.values():
            _set_grads(ps, gs)
            opt.step()
        for name in runs:
            _assert_same(*runs["dense"], *runs[name], (name, step))
        if step == 10:
            for name, live, src in (("dense->live", True, "dense"), ("live->dense", False, "live")):
                sd = copy.deepcopy(runs[src][1].state_dict())
                new(name, live, runs[src][0])[1].load_state_dict(sd)           # live: the flags are rebuilt from the moments
    st = runs["live"][1].live_stats()
    assert set(st) == {"color", "sdf"}, st                       # the weight's gradient was re-stored: dense kernel
    assert st["color"]["bricks"] == 90 and st["sdf"]["bricks"] == 6
    for name in ("live", "dense->live"):
        s = runs[name][1].live_stats()
        assert all(0 <= e["grad"] <= e["live"] <= e["bricks"] for e in s.values()), s
    assert 0 < st["color"]["live"] < 90, st                      # something was skipped in this test
    assert runs["dense"][1].live_stats() == {}


@pytest.mark.parametrize("case", ["weight_decay", "grad_layout", "misaligned"])
def test_live_mode_falls_back_to_the_dense_kernel(monkeypatch, case):
    from esr_nerf_amd import optimizer
    from esr_nerf_amd.optimizer import Adam
    monkeypatch.setattr(optimizer, "LIVE_MIN_NUMEL", 512)
    gen = torch.Generator(device=DEV).manual_seed(8)
    base = torch.randn(1, 6, 16, 12, 10, device=DEV, generator=gen).contiguous(memory_format=torch.channels_last_3d)

    def param():
        if case != "misaligned":
            return torch.nn.Parameter(base.clone(memory_format=torch.preserve_format))
        buf = torch.zeros(base.numel() + 4, device=DEV)
        t = buf[1:1 + base.numel()].view(1, 16, 12, 10, 6).permute(0, 4, 1, 2, 3)      # 4 bytes past a 16-byte boundary
        t.copy_(base)
        assert t.data_ptr() % 16 == 4 and t.is_contiguous(memory_format=torch.channels_last_3d)
        return torch.nn.Parameter(t)

    kw = dict(weight_decay=0.01) if case == "weight_decay" else {}
    pa, pb = param(), param()
    dense = Adam([pa], lr=0.1, betas=(B1, B2), **kw)
    live = Adam([pb], lr=0.1, betas=(B1, B2), live_bricks=True, zero_grads=True, **kw)
    for step in range(1, 6):
        g = torch.zeros(1, 16, 12, 10, 6, device=DEV)
        g[0, step] = torch.randn(12, 10, 6, device=DEV, generator=gen)
        g = g.permute(0, 4, 1, 2, 3)
        if case == "grad_layout":
            g = g.contiguous()                                    # logical order of a checkpointed or autograd gradient
        pa.grad, pb.grad = g.clone(memory_format=torch.preserve_format), g.clone(memory_format=torch.preserve_format)
        dense.step()
        live.step()
        assert torch.equal(pa, pb), (case, step)
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(dense.state[pa][key], live.state[pb][key]), (case, step, key)
        assert live.take_zeroed(pb.grad) is False, (case, step)
        assert torch.equal(pb.grad, pa.grad)                      # nothing zeroed it
    assert live.live_stats() == {}


def test_take_zeroed_marks_exactly_the_gradients_the_live_kernel_zeroed(monkeypatch):
    from esr_nerf_amd import optimizer
    from esr_nerf_amd.optimizer import Adam
    monkeypatch.setattr(optimizer, "LIVE_MIN_NUMEL", 512)
    ps = _params()
    opt = Adam(_groups(ps), betas=(B1, B2), live_bricks=True, zero_grads=True)
    gen = torch.Generator(device=DEV).manual_seed(4)
    _set_grads(ps, _grads(3, gen))
    opt.step()
    assert int(torch.count_nonzero(ps[0].grad)) == 0 and int(torch.count_nonzero(ps[1].grad)) == 0
    assert int(torch.count_nonzero(ps[2].grad)) > 0               # the dense way: not zeroed
    flat_view = ps[0].grad.permute(0, 2, 3, 4, 1).reshape(-1)     # any view of the same memory
    assert opt.take_zeroed(flat_view) is True and opt.take_zeroed(ps[0].grad) is False      # consumed
    assert opt.take_zeroed(ps[2].grad) is False
    _set_grads(ps, _grads(4, gen))
    opt.step()                                                    # a new step: new marks, the old ones are gone
    assert opt.take_zeroed(ps[1].grad) is True


# ---- trainer integration ------------------------------------------------------------------------------------------------
GRIDS = ("sdf", "off_color", "emo_color")


def _twin_update(m, opt, flat_before):
    """Dense esr_adam_step on clones of the grids, their moments and their gradients (taken before ``opt.step()``)."""
    from esr_nerf_amd.optimizer import _flat_storage
    out = {}
    for name in GRIDS:
        p = getattr(m, name).grid
        st = opt.state.get(p) or {}
        pc = p.detach().clone(memory_format=torch.preserve_format)
        mc = st["exp_avg"].clone(memory_format=torch.preserve_format) if st else torch.zeros_like(pc, memory_format=torch.preserve_format)
        vc = st["exp_avg_sq"].clone(memory_format=torch.preserve_format) if st else torch.zeros_like(pc, memory_format=torch.preserve_format)
        gc = p.grad.clone(memory_format=torch.preserve_format)
        out[name] = (pc, mc, vc, gc, int(st.get("step", 0)) + 1, opt.name2pg[name]["lr"])
    for name, (pc, mc, vc, gc, step, lr) in out.items():
        _lib, L = _L()
        _lib.check(L.esr_adam_step(_lib.ptr(_flat_storage(pc)), _lib.ptr(_flat_storage(gc)), _lib.ptr(_flat_storage(mc)),
                                   _lib.ptr(_flat_storage(vc)), None, C.c_int64(pc.numel()), C.c_float(lr), C.c_float(0.9),
                                   C.c_float(0.99), C.c_float(1e-8), C.c_float(0.0), step, _lib.stream_ptr(pc.device)),
                   "esr_adam_step")
    return out


def _checked_steps(m, step, opt, sampler, k):
    asked, take = [], opt.take_zeroed
    opt.take_zeroed = lambda t: asked.append(take(t)) or asked[-1]          # what the trainer step was told
    try:
        _checked_steps_(m, step, opt, sampler, k, asked)
    finally:
        del opt.take_zeroed


def _checked_steps_(m, step, opt, sampler, k, asked):
    for i in range(k):
        del asked[:]
        loss, grads = step.forward_loss_backward(sampler.sample(), 40.0)
        # behind an optimizer step every grid range is marked, and the step zeroes only the rest; the first call has none
        assert asked == [True] * 3 if i else not any(asked), (i, asked)
        step.assign_grads(grads)
        for name in GRIDS:                                        # the step consumed what the last opt.step() marked
            assert opt.take_zeroed(getattr(m, name).grid.grad) is False
        assert float(loss) == float(loss)
        twin = _twin_update(m, opt, step._flat)
        assert all(int(torch.count_nonzero(t[3])) > 0 for t in twin.values())
        opt.step()
        for name, (pc, mc, vc, _, n_step, _) in twin.items():
            p = getattr(m, name).grid
            assert torch.equal(p.detach(), pc), name
            assert torch.equal(opt.state[p]["exp_avg"], mc) and torch.equal(opt.state[p]["exp_avg_sq"], vc), name
            assert opt.state[p]["step"] == n_step
        assert int(torch.count_nonzero(step._flat[:step._n_grid])) == 0          # the live kernel's fill
        st = opt.live_stats()
        assert set(GRIDS) <= set(st), st
        for name in GRIDS:
            assert 0 < st[name]["grad"] <= st[name]["live"] <= st[name]["bricks"], (name, st[name])


def test_trainer_step_leaves_the_zero_fill_to_the_live_optimizer(monkeypatch):
    from test_gpu_train_loop import KEYS, LRS, _fresh
    from esr_nerf_amd import optimizer
    from esr_nerf_amd.config import AttrDict
    from esr_nerf_amd.data import BatchSampler
    from esr_nerf_amd.optimizer import create_optimizer_or_freeze_model
    from esr_nerf_amd.trainer import FineStep
    monkeypatch.setattr(optimizer, "LIVE_MIN_NUMEL", 1 << 18)    # the small scene's grids count as large
    m, sc = _fresh()
    torch.manual_seed(7)
    sampler = BatchSampler(AttrDict(system=dict(device=DEV, data_preload="cuda")), dict(sc.batch), KEYS, 512)
    sampler.shuffle()

    def live_opt():
        opt = create_optimizer_or_freeze_model(m, live_bricks=True, **LRS)
        opt.zero_grads = True
        return opt

    opt = live_opt()
    step = FineStep(m)
    assert step.zero_fill_by is None
    step.zero_fill_by = opt
    _checked_steps(m, step, opt, sampler, 6)

    # two forwards without an optimizer step between them: the second finds no marks and zeroes in full
    batch = sampler.sample()
    _, g1 = step.forward_loss_backward(batch, 40.0)
    n1 = {k: float(g1[f"{k}.grid"].double().norm()) for k in GRIDS}
    _, g2 = step.forward_loss_backward(batch, 40.0)
    for k in GRIDS:
        n2 = float(g2[f"{k}.grid"].double().norm())
        assert n1[k] > 0 and abs(n2 - n1[k]) <= 1e-3 * n1[k], (k, n1[k], n2)
    step.assign_grads(g2)
    opt.step()

    # the up-scaling event (fine.py:337-344): new grids, new optimizer, the same step object: it reallocates, zeroes in
    # full and goes on
    old = step._flat
    m.scale_volume_grid(160 * 160 * 40)
    opt = live_opt()
    step.zero_fill_by = opt
    _checked_steps(m, step, opt, sampler, 3)
    assert step._flat is not old and step._flat.numel() >= 13 * 160 * 160 * 40
