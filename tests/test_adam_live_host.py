"""Live-brick Adam without a GPU: the identity argument behind esr_adam_step_live in torch float32 with adam1's operation
order (csrc/adam.hip) -- a brick whose gradient was never non-zero and whose moments are zero keeps its bytes under the
dense update, so skipping it changes nothing, while a brick that was touched ONCE must go on being updated --, the
optimizer's interface of the mode (construction, state_dict keys, pickling, the environment switch), the C ABI's
declaration, and the generated code's registers."""
import os
import pickle
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRICK = 128
N_BRICKS = 60
STEPS = 40
LR, B1, B2, EPS = 0.1, 0.9, 0.99, 1e-8


def _adam1(p, g, m, v, plr, step):
    """adam1 with esr_adam_step's host scalars, every operation rounded to binary32 on its own; in place."""
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    one_m_b1, one_m_b2 = torch.tensor(1.0 - B1, dtype=torch.float32), torch.tensor(1.0 - B2, dtype=torch.float32)
    sqrt_bc2, neg_step = torch.tensor(bc2 ** 0.5, dtype=torch.float32), torch.tensor(-(LR / bc1), dtype=torch.float32)
    b1, b2, eps = (torch.tensor(x, dtype=torch.float32) for x in (B1, B2, EPS))
    m.copy_(m * b1 + g * one_m_b1)
    v.copy_(v * b2 + (g * g) * one_m_b2)
    denom = v.sqrt() / sqrt_bc2 + eps
    num = m * plr if plr is not None else m
    p.copy_(p + neg_step * (num / denom))


def _rows(t, idx):
    return t.view(N_BRICKS, BRICK)[idx]


def _step(state, g, plr, step, mode):
    """One update of (p, m, v, live) under ``mode``: dense, live (sticky flags) or the mutant that skips every brick whose
    gradient is zero in THIS step."""
    p, m, v, live = state
    nz = (g.view(N_BRICKS, BRICK) != 0).any(1)              # by value: -0.0 is zero
    if mode == "dense":
        _adam1(p, g, m, v, plr, step)
        return
    if mode == "live":
        live |= nz
        rows = live.nonzero().flatten()
    else:
        rows = nz.nonzero().flatten()
    pr, gr, mr, vr = (_rows(t, rows).clone() for t in (p, g, m, v))
    _adam1(pr, gr, mr, vr, None if plr is None else _rows(plr, rows), step)
    for t, r in ((p, pr), (m, mr), (v, vr)):
        t.view(N_BRICKS, BRICK)[rows] = r


def _gradients():
    """Bricks 0-9: a gradient in every step; 10-19: exactly once (step 3 + brick % 4) and never again; 20-29: a random
    subset per step, with -0.0 sprinkled in; 30-39: only ever -0.0; 40-59: never touched."""
    gen = torch.Generator().manual_seed(11)
    out = []
    for s in range(1, STEPS + 1):
        g = torch.zeros(N_BRICKS, BRICK)
        g[0:10] = torch.randn(10, BRICK, generator=gen) * 10.0 ** float(torch.randint(-6, 2, (1,), generator=gen))
        for b in range(10, 20):
            if s == 3 + b % 4:
                g[b, (7 * b) % BRICK] = 1e-3 * (b - 9)      # a single value of the brick
        pick = torch.rand(10, generator=gen) < 0.3
        g[20:30][pick] = torch.randn(int(pick.sum()), BRICK, generator=gen)
        g[20:30][:, ::5] *= -0.0
        g[30:40] = -0.0
        out.append(g.view(-1))
    return out


def _start(seed):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(N_BRICKS * BRICK, generator=gen)
    p[::17] = -0.0
    return [p, torch.zeros_like(p), torch.zeros_like(p), torch.zeros(N_BRICKS, dtype=torch.bool)]


@pytest.mark.parametrize("with_plr", [False, True])
def test_skipping_never_touched_bricks_is_the_identity(with_plr):
    grads = _gradients()
    plr = None
    if with_plr:
        plr = torch.rand(N_BRICKS * BRICK, generator=torch.Generator().manual_seed(5))
        plr[::3] = 0.0                                         # per-voxel rates are counts / max: zeros are common
    dense, live = _start(1), _start(1)
    for s, g in enumerate(grads, 1):
        _step(dense, g, plr, s, "dense")
        _step(live, g, plr, s, "live")
        for a, b, what in zip(dense[:3], live[:3], "pmv"):
            assert torch.equal(a, b), (what, s)
    assert live[3][:30].all() and not live[3][30:].any()       # -0.0 never makes a brick live
    assert torch.equal(live[0][30 * BRICK:], _start(1)[0][30 * BRICK:])


def test_a_skip_by_this_steps_gradient_is_caught():
    """The reference's dead "skip zero grad" idea: not sticky, so the moments of a brick touched once stop decaying and the
    parameter stops moving.  The comparison above must tell it from the dense update."""
    grads = _gradients()
    dense, mutant = _start(1), _start(1)
    differs = False
    for s, g in enumerate(grads, 1):
        _step(dense, g, None, s, "dense")
        _step(mutant, g, None, s, "mutant")
        differs |= not all(torch.equal(a, b) for a, b in zip(dense[:3], mutant[:3]))
    assert differs
    once = slice(10 * BRICK, 20 * BRICK)
    assert not torch.equal(dense[0][once], mutant[0][once]) and not torch.equal(dense[1][once], mutant[1][once])


def _cpu_params():
    return [torch.nn.Parameter(torch.zeros(1, 6, 4, 4, 4)), torch.nn.Parameter(torch.zeros(7, 3))]


def test_live_optimizer_constructs_and_keeps_the_dense_state_dict_and_its_mode_through_pickle():
    from esr_nerf_amd.optimizer import Adam
    live = Adam([dict(params=_cpu_params(), name="w")], lr=0.1, betas=(0.9, 0.99), live_bricks=True, zero_grads=True)
    dense = Adam([dict(params=_cpu_params(), name="w")], lr=0.1, betas=(0.9, 0.99))
    assert live.live_bricks and live.zero_grads and not dense.live_bricks and not dense.zero_grads
    a, b = live.state_dict(), dense.state_dict()
    assert set(a) == set(b) and a["state"] == b["state"] == {}
    assert [sorted(g) for g in a["param_groups"]] == [sorted(g) for g in b["param_groups"]]
    back = pickle.loads(pickle.dumps(live))
    assert back.live_bricks and back.zero_grads
    assert set(back.state_dict()) == set(b)
    plain = pickle.loads(pickle.dumps(dense))
    assert not plain.live_bricks and not plain.zero_grads
    assert live.live_stats() == {} and live.take_zeroed(torch.zeros(4)) is False


def test_state_of_the_mode_never_enters_optimizer_state():
    from esr_nerf_amd.optimizer import Adam
    ps = _cpu_params()
    opt = Adam(ps, live_bricks=True)
    opt.state[ps[0]] = dict(step=3, exp_avg=torch.ones_like(ps[0]), exp_avg_sq=torch.ones_like(ps[0]))
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    opt2 = Adam(_cpu_params(), live_bricks=True)
    opt2.load_state_dict(sd)
    assert set(opt2.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}


def test_set_pervoxel_lr_rejects_a_rate_that_is_not_finite_in_live_mode():
    from esr_nerf_amd.optimizer import Adam
    ps = _cpu_params()
    count = torch.ones_like(ps[0])
    Adam(ps, live_bricks=True).set_pervoxel_lr(count)
    bad = count.clone()
    bad[0, 0, 0, 0, 0] = float("inf")                        # inf / inf = nan
    with pytest.raises(ValueError):
        Adam(ps, live_bricks=True).set_pervoxel_lr(bad)
    Adam(ps).set_pervoxel_lr(bad)                              # the dense optimizer is as it was


def test_environment_switch_reaches_the_optimizer(monkeypatch):
    from esr_nerf_amd.optimizer import create_optimizer_or_freeze_model

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(3))
            self.net = torch.nn.Linear(2, 2)

    monkeypatch.delenv("ESR_ADAM_LIVE", raising=False)
    assert create_optimizer_or_freeze_model(M(), w=0.1, net=0.01).live_bricks is False
    monkeypatch.setenv("ESR_ADAM_LIVE", "1")
    opt = create_optimizer_or_freeze_model(M(), w=0.1, net=0.01)
    assert opt.live_bricks is True and opt.zero_grads is False
    assert [g["name"] for g in opt.param_groups] == ["w", "net"] and opt.param_groups[0]["betas"] == (0.9, 0.99)
    assert create_optimizer_or_freeze_model(M(), live_bricks=False, w=0.1).live_bricks is False
    monkeypatch.setenv("ESR_ADAM_LIVE", "0")
    assert create_optimizer_or_freeze_model(M(), w=0.1).live_bricks is False
    assert create_optimizer_or_freeze_model(M(), live_bricks=True, w=0.1).live_bricks is True


def test_header_declares_the_live_entries_and_ctypes_agrees():
    from esr_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    # the names only: tests/test_host.py checks every entry's restype and argument types against the header text
    assert {"esr_adam_step_live", "esr_brick_live_from_moments"} <= set(_lib.EXPORTS)
    assert "weight_decay" not in re.search(r"^int esr_adam_step_live\s*\(([^;]*)\);", header, re.M).group(1)


def test_live_kernel_uses_no_scratch_and_fits_eight_waves():
    """Compile-only, with the product's flags (tools/kernel_meta.py reads the assembler's resource comments): the dead-brick
    path is a pure stream and needs the occupancy."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta as km
    meta = km.kernel_meta(km.asm_of(os.path.join(ROOT, "esr_nerf_amd", "csrc", "adam.hip")))
    live = {k: v for k, v in meta.items() if "adam_live_kernel" in k}
    assert len(live) == 2, list(meta)                          # with and without the fused zero fill
    for name, k in list(live.items()) + [(n, v) for n, v in meta.items() if "live_from_moments" in n]:
        assert k.get("scratch", 0) == 0 and k.get("spill_v", 0) == 0 and k.get("spill_s", 0) == 0, (name, k)
        assert k.get("lds", 0) == 0, (name, k)
        assert k.get("vgpr", 999) + k.get("agpr", 0) <= 64 and k.get("occupancy") == 8, (name, k)


@pytest.mark.parametrize("marked", [(), ("sdf",), ("off_color",), ("emo_color",), ("sdf", "emo_color"), ("sdf", "off_color", "emo_color")])
def test_trainer_step_zeroes_everything_but_the_marked_grid_ranges(marked):
    """``_Step._zero_unmarked`` on CPU tensors: grid ranges the optimizer marked keep their bytes (they ARE zero: the live
    kernel's fill; ones here, to see them), everything else -- unmarked grids, the shard padding, the MLP part -- is
    zeroed, and asking consumes the marks."""
    from esr_nerf_amd.optimizer import Adam, _mem_key
    from esr_nerf_amd.trainer import FineStep
    step = FineStep(None)
    opt = Adam(_cpu_params(), live_bricks=True, zero_grads=True)
    step.zero_fill_by = opt
    step._flat = torch.ones(100)
    bounds = dict(sdf=(0, 10), off_color=(10, 40), emo_color=(40, 70))          # [70, 100): padding and MLP tensors
    views = {f"{k}.grid": step._flat[a:b].view(1, b - a) for k, (a, b) in bounds.items()}
    for k in marked:
        opt._zeroed.add(_mem_key(views[f"{k}.grid"]))
    step._zero_unmarked(views)
    want = torch.zeros(100)
    for k in marked:
        want[slice(*bounds[k])] = 1
    assert torch.equal(step._flat, want)
    assert not opt._zeroed
    step._flat.fill_(1)
    step._zero_unmarked(views)                                        # no optimizer step since: no marks, a full fill
    assert int(torch.count_nonzero(step._flat)) == 0
    for k in marked:                                                  # a reallocation only discards what is left over
        opt._zeroed.add(_mem_key(views[f"{k}.grid"]))
    step._flat.fill_(1)
    step._zero_unmarked(views, drop_only=True)
    assert not opt._zeroed and int(torch.count_nonzero(step._flat)) == 100
