"""Float64 restatement of the kernels that read and write every cell of every grid on every step -- the optimiser (csrc/adam.hip),
the regularisers (csrc/tv.hip) and the coarse stage's dense operators (csrc/dense.hip) -- with a plain binary32 torch emulation of
each operation and the input builders shared by tests/test_grid_ref64_host.py and tests/test_gpu_grid_ref64.py; never imported
by the product path.

Written from the formulas the kernel headers cite:
  adam          m' = b1 m + (1 - b1) g;  v' = b2 v + (1 - b2) g^2;  p' = p - (lr / bc1) (m' per_lr) / (sqrt(v') / sqrt(bc2) + eps),
                g <- g + wd p first under weight decay.  1 - b1, 1 - b2, sqrt(bc2) and -lr / bc1 are formed in double and rounded
                once; they enter as exact binary32 inputs.
  live adam     the same on every 128-value brick that is live or has a non-zero gradient; every other brick keeps its bits.  A
                live byte that was non-zero keeps its value, a new one is 1; stats += (bricks updated, bricks with a gradient);
                zero_grad zeroes exactly the bricks whose gradient had a non-zero value.
  tv_add_grad   grad += sum over the six neighbours of w clamp(p - neighbour, -1, 1), w = wy / 6 along j and wz / 6 along BOTH k and
                i, no term across a face; channels are stacked along the slowest axis; sparse mode skips cells with grad == 0.
  smooth tv     gradient_c = (s[+e_c] - s[-e_c]) / 2 / voxel on the interior of axis c, 0 on its boundary layer;
                err_c = mask ? bias + sum_abd w[a][b][d] gradient_c[clamp(x+a-1), clamp(y+b-1), clamp(z+d-1)] - gradient_c : 0;
                loss += weight / (3 masked_cells) sum err^2;  the backward (conv branch detached) adds
                coeff sum_c ([q-e_c interior] err_c[q-e_c] - [q+e_c interior] err_c[q+e_c]), coeff = -2 weight / (3 masked_cells) / 2 / voxel
                (times grad_out[0] when given), into grad_sdf.
  gauss3d       out[o] = sum_t w[t] in[clamp(o + t - r)] (replicate-padded cross-correlation); the adjoint is autograd of the float64
                forward, added into gin.
  central grad  [X, Y, Z, 3] central differences / 2 / voxel, 0 on the boundary layer; the adjoint is autograd of the float64 forward,
                added into gsdf.

Every entry returns, per output, (value, absref, zero): a value is checked as |got - value| <= K * U * absref + FLOOR (shade_ref64's
`compare`), with absref carried by lts_ref64's `Q` (its docstring has the algebra).  Sums of many products follow Q's sum rule --
E = sum E_i + r sum |v_i| with r roundings on the path of an addend -- evaluated with two float64 convolutions (values and
magnitudes): r = 28 for the 27-tap smoother (27 adds behind a product, the bias first), k^3 + 1 for the Gaussian, and k^3 + 2 for its
adjoint, which sums up to k^3 weights into `ws` before the product and then at most k^3 products.
  loss   absref = inv (sum E(e^2) + r sum e^2) + blocks (|loss0| + total): one rounding per addend of a thread (3 per trip), six shuffle
         levels, the four wave partials and the product by inv (r = 3 trips + 9), one float atomic per workgroup at a magnitude of
         at most |loss0| + total.
Beside the bound, `Ref.bits` lists what must hold bit for bit: name -> (mask, expected).  adam1 and `central` of tv.hip are
`fp contract(off)` with correctly rounded divide and square root, so wherever every intermediate is a normal number (or an exact 0)
p', m', v' and the gradient field equal the binary32 emulation bit for bit; values with a subnormal intermediate are held to the
float64 bound only and counted (`Ref.note`).  Untouched bricks, zero-gradient cells of the sparse mode, the live bytes, both
counters and every output of a call that must do nothing are bit checks too.
Consecutive steps: the reference of step k starts from the outputs of step k - 1 under test, so m and v are checked after every step
and no error is carried from one step's bound into the next.
No operation here decides on a computed value: the clamp of tv_add_grad is continuous and its g0 == 0 test reads an input.  Nothing
is exempted and the flip share is 0."""
from __future__ import annotations

import math

import torch

from lts_ref64 import Q, xsqrt, xwhere
from shade_ref64 import DEC_K, FLOOR, U, Ref, compare

F32, F64, I32 = torch.float32, torch.float64, torch.int32
BRICK, QUAD = 128, 4
THREADS = 4096 * 256             # esr_grid_for(n, 256, 256 * 16): the widest launch of these kernels
TINY = 2.0 ** -126


def f32(v):
    return float(torch.tensor(v, dtype=F32))


def t32(v):
    return torch.tensor(v, dtype=F32)


def bits(t):
    return t.contiguous().view(I32) if t.dtype == F32 else t


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _c(x, mode):
    """a scalar in the number system of `mode` ('q': Q over float64, '32': binary32)"""
    return t32(x) if mode == "32" else x


def _lift(x, mode):
    return Q(x.double()) if mode == "q" else x


def _out(q):
    return (q.v.detach(), q.E, None)


def _exact(t):
    """an output that must equal `t`: value t, absref 0 (the bit check rides in Ref.bits)"""
    return (t.double(), torch.zeros(t.shape, dtype=F64), None)


def _ref(out, bits_=None, note=None):
    r = Ref(out)
    r.bits, r.note = bits_ or {}, note or {}
    return r


# =======================================================================================================================
# adam
# =======================================================================================================================
def adam_scalars(cfg, step, mut=None):
    """the host scalars as adam_params forms them: double arithmetic, one rounding"""
    b1, b2, lr = f32(cfg["beta1"]), f32(cfg["beta2"]), f32(cfg["lr"])
    s = step - 1 if mut == "bias_correction_with_step_minus_1" else step
    bc1, bc2 = 1.0 - b1 ** s, 1.0 - b2 ** s
    neg = float(-(torch.tensor(lr, dtype=F64) / torch.tensor(bc1, dtype=F64)))
    return dict(b1=b1, b2=b2, eps=f32(cfg["eps"]), wd=f32(cfg["wd"]), omb1=f32(1.0 - b1), omb2=f32(1.0 - b2),
                sqrt_bc2=f32(math.sqrt(bc2)), neg=f32(neg))


def xsqrt32(a):
    """a correctly rounded binary32 square root (torch's own vectorised one is not): the float64 root, rounded once more"""
    return xsqrt(a) if isinstance(a, Q) else a.double().sqrt().float()


def adam_core(p, g, m, v, plr, S, mode, mut=None):
    """one adam1 per value; returns (p', m', v', every intermediate)"""
    c = lambda x: _c(x, mode)
    p, g, m, v, plr = [None if t is None else _lift(t, mode) for t in (p, g, m, v, plr)]
    inter = []

    def rec(x):
        inter.append(x)
        return x
    if S["wd"] != 0 and mut != "weight_decay_after_moments":
        g = rec(g + rec(p * c(S["wd"])))
    m2 = rec(rec(m * c(S["b1"])) + rec(g * c(S["omb1"])))
    v2 = rec(rec(v * c(S["b2"])) + rec(rec(g * g) * c(S["omb2"])))
    if mut == "eps_inside_sqrt":
        denom = rec(xsqrt32(v2 + c(S["eps"])) / c(S["sqrt_bc2"]))
    else:
        denom = rec(rec(rec(xsqrt32(v2)) / c(S["sqrt_bc2"])) + c(S["eps"]))
    num = m2 if plr is None else rec(m2 * plr)
    if mut == "per_lr_on_denominator" and plr is not None:
        num, denom = m2, denom * plr
    p2 = rec(p + rec(c(S["neg"]) * rec(num / denom)))
    if S["wd"] != 0 and mut == "weight_decay_after_moments":
        p2 = p2 + c(S["neg"]) * (p * c(S["wd"]))
    return p2, m2, v2, inter


def _normal(inputs, inter):
    ok = torch.ones(inputs[0].shape, dtype=torch.bool)
    for t in list(inputs) + list(inter):
        if t is not None:
            a = t.abs()
            ok &= ((a == 0) | (a >= TINY)) & torch.isfinite(t)
    return ok


def adam_ref_step(p, g, m, v, plr, S):
    """(out entries of one step, bit expectations) from binary32 state tensors"""
    qp, qm, qv, _ = adam_core(p, g, m, v, plr, S, "q")
    ep, em, ev, inter = adam_core(p, g, m, v, plr, S, "32")
    ok = _normal([p, g, m, v, plr], inter)
    return (qp, qm, qv), (ep, em, ev), ok


ADAM_STEPS = 3
ADAM_BASE = dict(n=1027, beta1=0.9, beta2=0.999, lr=0.1, eps=1e-8, wd=0.0, step=1, plr="rand", grad="randn", off=None, seed=0)
ADAM_NS = [1, 3, 4, 5, 127, 128, 129, 1027, 4 * 1048576 + 1203]
ADAM_CASES = {f"n{n}": dict(n=n, seed=n % 97) for n in ADAM_NS}
ADAM_CASES.update({f"off_{w}_plr": dict(off=w, seed=11 + i) for i, w in enumerate(("p", "g", "m", "v", "plr"))})
ADAM_CASES.update({f"off_{w}_noplr": dict(off=w, plr=None, seed=21 + i) for i, w in enumerate(("p", "g", "m", "v"))})
ADAM_CASES.update({f"step{s}": dict(step=s, seed=31 + i, n=129) for i, s in enumerate((1, 2, 1000, 100000))})
ADAM_CASES.update({
    "lr0": dict(lr=0.0, seed=41), "plr_zeros": dict(plr="zeros", seed=42), "noplr": dict(plr=None, seed=43, n=1029),
    "wd": dict(wd=0.01, seed=44), "wd_noplr_step1000": dict(wd=0.01, plr=None, step=1000, seed=45),
    "eps0": dict(eps=0.0, grad="moderate", seed=46), "grad_zero": dict(grad="zero", seed=47), "grad_wide": dict(grad="wide", seed=48),
    "m_opposes_g": dict(grad="opposite", seed=49), "wd_off_m": dict(wd=0.01, off="m", seed=50),
})
ADAM_BIG = f"n{ADAM_NS[-1]}"
_CACHE = {}


def case_adam(name):
    if ("adam", name) in _CACHE:
        return _CACHE[("adam", name)]
    cfg = dict(ADAM_BASE, **ADAM_CASES[name])
    n, g_ = cfg["n"], _gen(1000 + cfg["seed"])
    rn = lambda: torch.randn(n, generator=g_)
    p, m, v = rn(), rn() * 0.1, rn().square() * 0.01
    kind = cfg["grad"]
    gs = []
    for k in range(ADAM_STEPS):
        if kind == "zero":
            g = torch.zeros(n)
        elif kind == "wide":                                           # magnitudes 1e-20 .. 1e18, mixed signs
            g = torch.sign(rn()) * torch.pow(10.0, torch.rand(n, generator=g_) * 38 - 20)
            g[0], g[-1] = 1e-20, -1e18
        elif kind == "moderate":
            g = rn() * 0.5
        else:
            g = rn() * torch.pow(10.0, torch.randint(-4, 2, (n,), generator=g_).float())
        gs.append(g)
    if kind == "opposite":
        m = -gs[0].clone()
    if kind == "zero":
        m[::3], v[::3] = 0.0, 0.0                                       # (the identity of the live-brick form among them)
    if cfg["eps"] == 0.0:
        v = v + 1e-6                                                    # eps = 0 only with v > 0 everywhere
    plr = None
    if cfg["plr"] is not None:
        plr = torch.rand(n, generator=g_) * 2
        if cfg["plr"] == "zeros":
            plr[::2] = 0.0
    vec = cfg["off"] is None
    n4 = n // 4
    census = {"vector kernel" if vec else "scalar kernel", f"step {cfg['step']}", f"lr {cfg['lr']}", f"n % 4 = {n % 4}"}
    if vec and n % 4:
        census.add("scalar tail")
    if vec and n4 == 0:
        census.add("no whole float4")
    if vec and n4 > THREADS:
        census.add("second trip")
    if plr is None:
        census.add("per_lr NULL")
    elif bool((plr == 0).any()):
        census.add("per_lr zeros")
    if cfg["wd"]:
        census.add("weight decay")
    if cfg["eps"] == 0 and bool((v > 0).all()):
        census.add("eps 0")
    if all(bool((g == 0).all()) for g in gs):
        census.add("zero gradient")
    if float(gs[0].abs().max()) >= 1e17 and float(gs[0].abs().min()) <= 1e-19:
        census.add("gradient 1e-20 .. 1e18")
    if torch.equal(m, -gs[0]):
        census.add("m = -g")
    if cfg["off"]:
        census.add(f"{cfg['off']} offset by 4 bytes")
    claims = set(census)
    sample = None
    if n > THREADS:                                                      # (verify_adam)
        sample = torch.unique(torch.cat([torch.arange(min(4 * THREADS, n4 * 4), n), torch.randperm(n, generator=g_)[:n // 20]]))
    inp = dict(cfg, name=name, p=p, m=m, v=v, gs=gs, per_lr=plr, vec=vec, census=census, claims=claims, sample=sample)
    _CACHE[("adam", name)] = inp
    return inp


def emu_adam(inp, mut=None):
    p, m, v, plr, n = inp["p"], inp["m"], inp["v"], inp["per_lr"], inp["n"]
    n4, got = n // 4, {}
    for k in range(ADAM_STEPS):
        S = adam_scalars(inp, inp["step"] + k, mut)
        pl = plr
        if mut == "float4_w_takes_z_per_lr" and plr is not None and inp["vec"]:
            pl, i = plr.clone(), torch.arange(3, max(n4 * 4, 3), 4)
            pl[i] = plr[i - 1]
        p2, m2, v2, _ = adam_core(p, inp["gs"][k], m, v, pl, S, "32", mut)
        if mut == "scalar_tail_skipped" and inp["vec"]:
            p2[n4 * 4:], m2[n4 * 4:], v2[n4 * 4:] = p[n4 * 4:], m[n4 * 4:], v[n4 * 4:]
        p, m, v = p2, m2, v2
        got.update({f"p{k + 1}": p, f"m{k + 1}": m, f"v{k + 1}": v})
    return got


def verify_adam(inp, got, K):
    """Every value against float64.  The 4.2 M case holds every value to the emulation's bits and evaluates the float64 reference on
    the values of the second trip, the scalar tail, every value with a subnormal intermediate and a random 5 % of the rest
    (the outputs `<name>@sample`), to keep the host reference to a few seconds."""
    out, bits_, flushed, sub = {}, {}, 0, 0
    p, m, v, plr = inp["p"], inp["m"], inp["v"], inp["per_lr"]
    got = dict(got)
    for k in range(ADAM_STEPS):
        S = adam_scalars(inp, inp["step"] + k)
        g = inp["gs"][k]
        ep, em, ev, inter = adam_core(p, g, m, v, plr, S, "32")
        ok = _normal([p, g, m, v, plr], inter)
        sub += 3 * int((~ok).sum())
        idx, tag = None, ""
        if inp.get("sample") is not None:
            idx, tag = torch.unique(torch.cat([inp["sample"], torch.nonzero(~ok).reshape(-1)])), "@sample"
        pick = lambda t: t if (idx is None or t is None) else t[idx]
        qs = adam_core(pick(p), pick(g), pick(m), pick(v), pick(plr), S, "q")[:3]
        nxt = []
        for nm, q, e in zip("pmv", qs, (ep, em, ev)):
            key = f"{nm}{k + 1}"
            t = got[key].cpu().float().reshape(-1)
            nxt.append(t)
            out[key + tag] = _out(q)
            got[key + tag] = pick(t)
            bits_[key] = (ok, e)
            flushed += int((bits(t) != bits(e))[~ok].sum())
        p, m, v = nxt
        if not all(bool(torch.isfinite(t).all()) for t in nxt):
            break
    r = _ref(out, bits_, {"values with a subnormal intermediate": sub, "of which differ from the unflushed emulation": flushed})
    return (r,) + _judge(r, got, K)


# ---- live bricks ------------------------------------------------------------------------------------------------------
LIVE_STEPS = 2
LIVE_BIG_N = (131072 + 2) * QUAD * BRICK + 3 * BRICK + 7
LIVE_NS = [5, 128, 512, 513, 512 * 3 + 128 * 3 + 5, 128 * 37 + 5]
LIVE_CASES = {}
for _i, _n in enumerate(LIVE_NS):
    for _z in (0, 1):
        LIVE_CASES[f"n{_n}_z{_z}"] = dict(n=_n, zero_grad=_z, stats=(_i + _z) % 2 == 0, plr=(_i % 2 == 0), tail="nz" if _z else "mixed",
                                          seed=_i * 2 + _z)
LIVE_CASES["n4741_z1_tail_dead"] = dict(n=128 * 37 + 5, zero_grad=1, stats=True, plr=False, tail="dead", seed=20)
LIVE_CASES["big"] = dict(n=LIVE_BIG_N, zero_grad=1, stats=True, plr=False, tail="nz", seed=30, sparse=True)
ROLES = ("nz", "dead", "live_zero_grad", "dead_negzero", "last_lane", "live255_nz", "dead", "nz_first_lane")
STATS0 = (5, 11)


def _n_bricks(n):
    return (n + BRICK - 1) // BRICK


def case_live(name):
    """Small cases hold full tensors.  The big one holds brick lists: p is a tile repeated, m, v and the gradients are zero outside
    the listed bricks, so neither the host nor the reference ever forms the 67 M values."""
    if ("live", name) in _CACHE:
        return _CACHE[("live", name)]
    cfg = {**ADAM_BASE, "step": 3, "sparse": False, **LIVE_CASES[name]}
    n, g_ = cfg["n"], _gen(2000 + cfg["seed"])
    nb = _n_bricks(n)
    ragged = n % BRICK
    census = set()
    if cfg["sparse"]:
        k = nb // 100
        pick = lambda: torch.sort(torch.randperm(nb - 4, generator=g_)[:k])[0]
        tailb = torch.arange(nb - 4, nb)                               # the three whole bricks and the ragged one behind the last quad
        lists = {}
        live0 = torch.zeros(nb, dtype=torch.uint8)
        lb = torch.cat([pick(), tailb[1:2]])
        live0[lb] = 1
        live0[lb[::7]] = 255
        lists["m"] = (lb, torch.randn(len(lb), BRICK, generator=g_) * 0.1)
        lists["v"] = (lb, torch.randn(len(lb), BRICK, generator=g_).square() * 0.01)
        for s in range(LIVE_STEPS):
            gb = torch.cat([pick(), tailb[[0, 3]] if s == 0 else tailb[2:3]])
            gv = torch.randn(len(gb), BRICK, generator=g_) * 0.3
            gv[::5] = 0.0
            gv[::5, BRICK - 1] = 0.25                                  # a fifth of them: the last lane only
            gv[1::9] = -0.0                                            # listed, yet dead: -0.0 only
            if s == 0:
                gv[-1] = 0.0
                gv[-1, ragged - 1] = -0.5                              # the ragged brick: its last value only
            lists[f"g{s}"] = (gb, gv)
        inp = dict(cfg, name=name, nb=nb, lists=lists, live=live0, tile=torch.randn(4099, generator=g_), per_lr=None)
        census |= {"second trip", "about 1 % of the bricks touched"}
    else:
        role = [ROLES[(b + cfg["seed"]) % len(ROLES)] for b in range(nb)]
        if ragged and nb > 0:
            role[-1] = {"nz": "ragged_last_value", "dead": "dead_negzero", "mixed": role[-1]}[cfg["tail"]]
        p, m, v = torch.randn(n, generator=g_), torch.zeros(n), torch.zeros(n)
        live0, gs = torch.zeros(nb, dtype=torch.uint8), [torch.zeros(n) for _ in range(LIVE_STEPS)]
        for b, r in enumerate(role):
            lo, hi = b * BRICK, min((b + 1) * BRICK, n)
            w = hi - lo
            if r.startswith("live"):
                live0[b] = 255 if "255" in r else 1
                m[lo:hi], v[lo:hi] = torch.randn(w, generator=g_) * 0.1, torch.randn(w, generator=g_).square() * 0.01
            for s in range(LIVE_STEPS):
                rs = r if s == 0 else role[(b + 3) % nb] if b < nb - 1 or not ragged else "live_zero_grad"
                if rs in ("nz", "live255_nz"):
                    gs[s][lo:hi] = torch.randn(w, generator=g_) * 0.3
                    gs[s][lo:hi:3] = 0.0
                elif rs == "dead_negzero":
                    gs[s][lo:hi:2] = -0.0
                elif rs in ("last_lane", "ragged_last_value"):
                    gs[s][hi - 1] = 0.25
                elif rs == "nz_first_lane":
                    gs[s][lo] = -1e-3
        plr = torch.rand(n, generator=g_) * 2 if cfg["plr"] else None
        inp = dict(cfg, name=name, nb=nb, p=p, m=m, v=v, gs=gs, live=live0, per_lr=plr)
    # census, from the data
    live = inp["live"]
    for s in range(LIVE_STEPS):
        nz = live_nz_bricks(inp, s)
        if bool(((live != 0) & ~nz).any()):
            census.add("already live, zero gradient")
        if bool((live == 255).any()):
            census.add("live byte 255")
        if bool((~nz & (live == 0)).any()):
            census.add("dead brick")
        if s == 0 and ragged and bool(nz[-1]):
            census.add("gradient only in the ragged tail")
        live = torch.where(live != 0, live, nz.to(torch.uint8))
    if not cfg["sparse"]:
        g0 = inp["gs"][0]
        gb = torch.nn.functional.pad(g0, (0, nb * BRICK - n)).reshape(nb, BRICK)
        if bool(((gb[:, :BRICK - 1] == 0).all(1) & (gb[:, BRICK - 1] != 0)).any()):
            census.add("gradient only in the last lane")
        dead = ~live_nz_bricks(inp, 0)
        if bool((torch.signbit(gb) & (gb == 0)).any(1)[dead].any()):
            census.add("-0.0 in a dead brick")
    else:
        gb, gv = inp["lists"]["g0"]
        census |= {"gradient only in the last lane", "-0.0 in a dead brick"}
        assert bool(((gv[:, :BRICK - 1] == 0).all(1) & (gv[:, BRICK - 1] != 0)).any()) and bool((torch.signbit(gv) & (gv == 0)).all(1).any())
    census.add(f"zero_grad {cfg['zero_grad']}")
    census.add("stats given" if cfg["stats"] else "stats NULL")
    census.add("per_lr given" if inp["per_lr"] is not None else "per_lr NULL")
    if n // (QUAD * BRICK) and n % (QUAD * BRICK):
        census.add("whole quads and a tail")
    if n % (QUAD * BRICK) >= BRICK and ragged:
        census.add("whole bricks and a ragged one in the tail")
    if n // (QUAD * BRICK) > THREADS // 32:
        census.add("second trip")
    inp["census"], inp["claims"] = census, set(census)
    _CACHE[("live", name)] = inp
    return inp


def live_nz_bricks(inp, s):
    """bool[nb]: the bricks whose gradient of step s has a non-zero value"""
    nb, n = inp["nb"], inp["n"]
    if inp["sparse"]:
        gb, gv = inp["lists"][f"g{s}"]
        valid = (gb[:, None] * BRICK + torch.arange(BRICK)[None]) < n
        out = torch.zeros(nb, dtype=torch.bool)
        out[gb] = ((gv != 0) & valid).any(1)
        return out
    g = torch.nn.functional.pad(inp["gs"][s], (0, nb * BRICK - n)).reshape(nb, BRICK)
    return (g != 0).any(1)


def live_plan(inp, mut=None):
    """per step: (todo bricks, nz bricks, live bytes after, element indices of the todo bricks) -- from the inputs alone"""
    plan, live, n = [], inp["live"], inp["n"]
    for s in range(LIVE_STEPS):
        nz = live_nz_bricks(inp, s)
        todo = nz | (live != 0)
        if mut == "live_brick_with_zero_gradient_skipped":
            todo = nz
        if mut == "ragged_brick_dropped" and n % BRICK:
            todo = todo.clone()
            todo[-1] = False
        after = torch.where(live != 0, live, todo.to(torch.uint8))
        b = torch.nonzero(todo).reshape(-1)
        sel = (b[:, None] * BRICK + torch.arange(BRICK)[None]).reshape(-1)
        plan.append(dict(todo=todo, nz=nz, live=after, sel=sel[sel < n]))
        live = after
    return plan


def live_vals(inp, name, sel):
    """the initial values of tensor `name` ('p', 'm', 'v', 'g0', 'g1', 'per_lr') at element indices `sel`"""
    if not inp["sparse"]:
        t = inp["gs"][int(name[1])] if name[0] == "g" else inp[name]
        return None if t is None else t[sel]
    if name == "per_lr":
        return None
    if name == "p":
        return inp["tile"][sel % inp["tile"].numel()]
    bl, vals = inp["lists"][name]
    out = torch.zeros(sel.numel())
    b = sel // BRICK
    pos = torch.searchsorted(bl, b).clamp(max=bl.numel() - 1)
    hit = bl[pos] == b
    out[hit] = vals[pos[hit], sel[hit] % BRICK]
    return out


def live_full(inp, device):
    """the full state on `device`: dict p, m, v, g0, g1, per_lr, live"""
    n = inp["n"]
    if not inp["sparse"]:
        st = {k: inp[k].to(device) for k in ("p", "m", "v", "live")}
        st.update({f"g{s}": g.to(device) for s, g in enumerate(inp["gs"])})
        st["per_lr"] = None if inp["per_lr"] is None else inp["per_lr"].to(device)
        return st
    tile = inp["tile"].to(device)
    st = dict(p=tile[torch.arange(n, device=device) % tile.numel()], live=inp["live"].to(device), per_lr=None)
    for k, (bl, vals) in inp["lists"].items():
        t = torch.zeros(n, device=device)
        idx = (bl[:, None] * BRICK + torch.arange(BRICK)[None]).reshape(-1)
        keep = idx < n
        t[idx[keep].to(device)] = vals.reshape(-1)[keep].to(device)
        st[k] = t
    return st


def live_collect(inp, s, plan, before, after, stats):
    """what a step left, in the gathered form the reference reads: works on either device"""
    dev = after["p"].device
    sel = plan[s]["sel"].to(dev)
    keep = torch.ones(inp["n"], dtype=torch.bool, device=dev)
    keep[sel] = False
    got = {f"{k}{s + 1}": after[k][sel].cpu() for k in "pmv"}
    rest = all(bool((bits(after[k]) == bits(before[k]))[keep].all()) for k in "pmv")
    got[f"rest{s + 1}"] = torch.tensor([1.0 if rest else 0.0])
    got[f"live{s + 1}"] = after["live"].cpu()
    gb, ga = bits(before[f"g{s}"]), bits(after[f"g{s}"])
    nzb = plan[s]["nz"].to(dev)
    nze = nzb.repeat_interleave(BRICK)[:inp["n"]]
    if inp["zero_grad"]:
        ok = bool((ga[nze] == 0).all()) and bool((ga == gb)[~nze].all())
    else:
        ok = bool((ga == gb).all())
    got[f"grad{s + 1}"] = torch.tensor([1.0 if ok else 0.0])
    if stats is not None:
        got[f"stats{s + 1}"] = stats.cpu().clone()
    return got


def emu_adam_live(inp, mut=None):
    plan_true, plan = live_plan(inp), live_plan(inp, mut)
    got = {}
    stats = torch.tensor(STATS0, dtype=torch.int64) if inp["stats"] else None
    if inp["sparse"]:                                                   # gathered throughout
        assert mut is None
        prev = {}
        for s in range(LIVE_STEPS):
            sel = plan[s]["sel"]
            cur = {k: live_vals(inp, k, sel) for k in "pmv"}
            if s:
                pos = torch.searchsorted(sel, plan[s - 1]["sel"])
                for k in "pmv":
                    cur[k][pos] = prev[k]
            S = adam_scalars(inp, inp["step"] + s)
            p2, m2, v2, _ = adam_core(cur["p"], live_vals(inp, f"g{s}", sel), cur["m"], cur["v"], None, S, "32")
            prev = dict(p=p2, m=m2, v=v2)
            got.update({f"p{s + 1}": p2, f"m{s + 1}": m2, f"v{s + 1}": v2, f"rest{s + 1}": torch.ones(1), f"grad{s + 1}": torch.ones(1),
                        f"live{s + 1}": plan[s]["live"]})
            if stats is not None:
                stats = stats + torch.tensor([int(plan[s]["todo"].sum()), int(plan[s]["nz"].sum())])
                got[f"stats{s + 1}"] = stats
        return got
    st = live_full(inp, "cpu")
    st = {k: (t.clone() if t is not None else None) for k, t in st.items()}
    n = inp["n"]
    for s in range(LIVE_STEPS):
        before = {k: (t.clone() if t is not None else None) for k, t in st.items()}
        S = adam_scalars(inp, inp["step"] + s)
        p2, m2, v2, _ = adam_core(st["p"], st[f"g{s}"], st["m"], st["v"], st["per_lr"], S, "32")
        te = plan[s]["todo"].repeat_interleave(BRICK)[:n]
        st["p"], st["m"], st["v"] = torch.where(te, p2, st["p"]), torch.where(te, m2, st["m"]), torch.where(te, v2, st["v"])
        st["live"] = torch.where(st["live"] != 0, st["live"], plan[s]["todo"].to(torch.uint8))
        if inp["zero_grad"]:
            ze = plan[s]["nz"].repeat_interleave(BRICK)[:n]
            if mut == "gradient_zeroed_in_dead_brick":
                ze = torch.ones_like(ze)
            st[f"g{s}"] = torch.where(ze, torch.zeros(n), st[f"g{s}"])
        if stats is not None:
            stats = stats + torch.tensor([int(plan[s]["todo"].sum()), int(plan[s]["nz"].sum())])
        got.update(live_collect(inp, s, plan_true, before, st, stats))
    return got


def verify_adam_live(inp, got, K):
    plan = live_plan(inp)
    out, bits_, prev = {}, {}, {}
    stats = torch.tensor(STATS0, dtype=torch.int64)
    for s in range(LIVE_STEPS):
        sel = plan[s]["sel"]
        cur = {k: live_vals(inp, k, sel) for k in "pmv"}
        if s:
            pos = torch.searchsorted(sel, plan[s - 1]["sel"])
            for k in "pmv":
                cur[k][pos] = prev[k]
        S = adam_scalars(inp, inp["step"] + s)
        qs, es, ok = adam_ref_step(cur["p"], live_vals(inp, f"g{s}", sel), cur["m"], cur["v"], live_vals(inp, "per_lr", sel), S)
        for nm, q, e in zip("pmv", qs, es):
            out[f"{nm}{s + 1}"] = _out(q)
            bits_[f"{nm}{s + 1}"] = (ok, e)
        one = torch.ones(1)
        for nm, t in ((f"rest{s + 1}", one), (f"grad{s + 1}", one), (f"live{s + 1}", plan[s]["live"])):
            out[nm] = _exact(t)
            bits_[nm] = (torch.ones(t.shape, dtype=torch.bool), t)
        if inp["stats"]:
            stats = stats + torch.tensor([int(plan[s]["todo"].sum()), int(plan[s]["nz"].sum())])
            out[f"stats{s + 1}"] = _exact(stats)
            bits_[f"stats{s + 1}"] = (torch.ones(2, dtype=torch.bool), stats)
        prev = {k: got[f"{k}{s + 1}"].cpu().float().reshape(-1) for k in "pmv"}
        if any(prev[k].shape != cur[k].shape or not bool(torch.isfinite(prev[k]).all()) for k in "pmv"):
            break
    r = _ref(out, bits_)
    for k_ in list(got):
        if k_ not in out:
            got = {a: b for a, b in got.items() if a != k_}
    for k_ in list(out):
        if k_ not in got:
            del out[k_], bits_[k_]
    return (r,) + _judge(r, got, K)


# ---- live flags from loaded moments -----------------------------------------------------------------------------------
def case_from_moments(n):
    g_ = _gen(3000 + n)
    nb = _n_bricks(n)
    m, v, live0 = torch.zeros(n), torch.zeros(n), torch.zeros(nb, dtype=torch.uint8)
    census = set()
    for b in range(nb):
        lo, hi = b * BRICK, min((b + 1) * BRICK, n)
        r = ("m", "none", "v_last", "negzero", "was255", "m_first")[(b + n) % 6]
        if b == nb - 1 and n % BRICK:
            r = "v_last"
        if r == "m":
            m[lo:hi] = torch.randn(hi - lo, generator=g_)
        elif r == "v_last":
            v[hi - 1] = 1e-30
            census.add("only the last value of a brick" if hi - lo == BRICK else "only the last value of the ragged brick")
        elif r == "negzero":
            m[lo:hi], v[lo:hi:2] = -0.0, -0.0
            census.add("-0.0 only")
        elif r == "was255":
            live0[b] = 255
            census.add("live byte 255")
        elif r == "m_first":
            m[lo] = -1e-30
    return dict(name=f"n{n}", n=n, nb=nb, m=m, v=v, live=live0, census=census, claims=set(census))


def _moments_expect(inp, mut=None):
    nb, n = inp["nb"], inp["n"]
    pad = lambda t: torch.nn.functional.pad(t, (0, nb * BRICK - n)).reshape(nb, BRICK)
    nz = (pad(inp["m"]) != 0).any(1) | (pad(inp["v"]) != 0).any(1)
    if mut == "ragged_brick_dropped" and n % BRICK:
        nz[-1] = False
    return torch.where(inp["live"] != 0, inp["live"], nz.to(torch.uint8))


def emu_from_moments(inp, mut=None):
    return {"live": _moments_expect(inp, mut)}


def verify_from_moments(inp, got, K):
    t = _moments_expect(inp)
    r = _ref({"live": _exact(t)}, {"live": (torch.ones(t.shape, dtype=torch.bool), t)})
    return (r,) + _judge(r, got, K)


# =======================================================================================================================
# stencils: grids, neighbours, census
# =======================================================================================================================
GRIDS = {"1x1x1": (1, 1, 1), "1x1x7": (1, 1, 7), "2x2x2": (2, 2, 2), "2x5x1": (2, 5, 1), "3x3x3": (3, 3, 3), "5x4x3": (5, 4, 3),
         "9x7x6": (9, 7, 6), "1x2x2": (1, 2, 2), "129x128x64": (129, 128, 64)}
BIG_GRID = "129x128x64"
SMALL_GRIDS = [g for g in GRIDS if g != BIG_GRID]


def nbr(t, axis, d):
    """the neighbour at +d along `axis`, replicated at the ends (a face cell reads itself)"""
    n = t.shape[axis]
    return t.index_select(axis, (torch.arange(n) + d).clamp(0, n - 1))


def pos(shape, axis):
    s = [1] * len(shape)
    s[axis] = shape[axis]
    return torch.arange(shape[axis]).reshape(s).expand(shape)


def grid_census(dims):
    on = sum(((pos(dims, a) == 0) | (pos(dims, a) == dims[a] - 1)).int() for a in range(3))
    c = {name for k, name in ((3, "corner"), (2, "edge"), (1, "face"), (0, "interior")) if bool((on == k).any())}
    if 1 in dims:
        c.add("axis of length 1")
    if 2 in dims:
        c.add("axis of length 2")
    if "interior" not in c:
        c.add("no interior cell")
    if dims[0] * dims[1] * dims[2] > THREADS:
        c.add("second trip")
    if all(d < 3 for d in dims):
        c.add("every axis shorter than r = 3")
    return c


def xclamp1(a):
    """clamp(a, -1, 1): continuous, so the error passes inside and dies outside the band"""
    if isinstance(a, Q):
        dead = a.v.detach().abs() > 1 + DEC_K * U * a.E
        return Q(a.v.clamp(-1, 1), torch.where(dead, torch.zeros_like(a.E), a.E))
    return a.clamp(-1, 1)


def xhalf(a):
    return a.scale2(0.5) if isinstance(a, Q) else a * 0.5


def pad_rep(x, r):
    """replicate padding by r on the three last axes (any r, any size)"""
    for a in range(x.dim() - 3, x.dim()):
        n = x.shape[a]
        x = x.index_select(a, torch.arange(-r, n + r).clamp(0, n - 1))
    return x


def corr3(x, w, r):
    """replicate-padded cross-correlation of [.., X, Y, Z] with w [k, k, k], in x's dtype"""
    lead = x.shape[:-3]
    y = torch.nn.functional.conv3d(pad_rep(x.reshape(-1, 1, *x.shape[-3:]), r), w.to(x.dtype)[None, None])
    return y.reshape(*lead, *x.shape[-3:])


def _wmut(w, mut):
    return w.permute(2, 1, 0).contiguous() if mut == "conv_taps_transposed_xz" else w


# ---- tv_add_grad ------------------------------------------------------------------------------------------------------
TV_C = 3
TV_CASES = {f"{g}_{'dense' if d else 'sparse'}": (g, d) for g in GRIDS for d in (1, 0)}


def case_tv(name):
    if ("tv", name) in _CACHE:
        return _CACHE[("tv", name)]
    gname, dense = TV_CASES[name]
    X, Y, Z = GRIDS[gname]
    C = 1 if gname == BIG_GRID else TV_C
    g_ = _gen(4000 + sum(map(ord, name)))
    param = torch.rand(C, X, Y, Z, generator=g_) * 1.5 + 1e3 * torch.arange(C).float().reshape(C, 1, 1, 1)   # a jump of 1e3 per seam
    census = grid_census((X, Y, Z))
    if (X, Y, Z) >= (9, 7, 6):
        for c in range(C):
            for cell, d in (((1, 1, 1), 1.0), ((4, 1, 1), -1.0), ((7, 1, 1), 5.0), ((2, 4, 3), -4.5), ((6, 4, 3), 0.0)):
                x, y, z = cell
                v0 = 0.25 + 1e3 * c                                     # (v0 and v0 - d are binary32 numbers: the difference is exact)
                param[c, x, y, z] = v0
                for dx, dy, dz in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
                    param[c, x + dx, y + dy, z + dz] = v0 - d
    grad = torch.randn(C, X, Y, Z, generator=g_) * 0.1
    if not dense:
        flat = grad.reshape(-1)
        flat[::3] = 0.0
        flat[1::6] = -0.0
    wy, wz = f32(0.37), f32(0.91)
    inp = dict(name=name, param=param, grad=grad, dims=(X, Y, Z), C=C, dense=dense, wx=f32(0.5), wy=wy, wz=wz)
    # the census of the planted differences, from the data
    for a in (1, 2, 3):
        for d in (-1, 1):
            diff = (param.double() - nbr(param, a, d).double())[(pos(param.shape, a) != (0 if d < 0 else param.shape[a] - 1))]
            if bool((diff == 1).any()) and bool((diff == -1).any()):
                census.add(f"difference exactly +-1 (axis {a}, {d:+d})")
            if bool((diff > 1).any()) and bool((diff < -1).any()):
                census.add(f"difference beyond +-1 (axis {a}, {d:+d})")
            if bool((diff == 0).any()):
                census.add(f"equal neighbours (axis {a}, {d:+d})")
    if C > 1:
        census.add("channel seam with a jump of 1e3")
    if wy != wz:
        census.add("wy != wz")
    if not dense and bool((torch.signbit(grad) & (grad == 0)).any()) and bool((~torch.signbit(grad) & (grad == 0)).any()):
        census.add("-0.0 and +0.0 gradients")
    census.add("dense" if dense else "sparse")
    inp["census"], inp["claims"] = census, set(census)
    _CACHE[("tv", name)] = inp
    return inp


def _tv_any(inp, mode, mut=None):
    param, g0 = inp["param"], inp["grad"]
    wy6, wz6 = float(t32(inp["wy"]) / 6), float(t32(inp["wz"]) / 6)      # the entry's own binary32 divides
    P = _lift(param, mode)
    flat = param.reshape(1, -1, *param.shape[2:])                       # the seam-blind view of the slowest axis
    g = None
    for axis, d, w in ((3, -1, wz6), (3, 1, wz6), (2, -1, wy6), (2, 1, wy6), (1, -1, wz6), (1, 1, wz6)):
        if axis == 1 and mut == "wy_on_i_axis":
            w = wy6
        src = flat if (axis == 1 and mut == "seam_neighbour_read") else param
        has = pos(src.shape, axis) != (0 if d < 0 else src.shape[axis] - 1)
        nb_ = nbr(src, axis, d).reshape(param.shape)
        has = has.reshape(param.shape)
        diff = P - _lift(nb_, mode)
        cl = diff if mut == "clamp_dropped" else xclamp1(diff)
        term = xwhere(has, cl * _c(w, mode), Q(torch.zeros(param.shape, dtype=F64)) if mode == "q" else torch.zeros(param.shape))
        g = term if g is None else g + term
    out = _lift(g0, mode) + g
    skip = torch.zeros(param.shape, dtype=torch.bool)
    if not inp["dense"] and mut != "sparse_updates_zero_gradient_cells":
        skip = g0 == 0
        out = xwhere(skip, _lift(g0, mode), out)
    return out, skip


def emu_tv(inp, mut=None):
    return {"grad": _tv_any(inp, "32", mut)[0]}


def verify_tv(inp, got, K):
    q, skip = _tv_any(inp, "q")
    b = {"grad": (skip, inp["grad"])}
    if inp["dims"] == (1, 1, 1):
        b = {"grad": (torch.ones_like(skip), inp["grad"])}              # no neighbour anywhere: bit-identical
    r = _ref({"grad": _out(q)}, b)
    return (r,) + _judge(r, got, K)


# ---- central differences (shared by the smoothed-gradient term and the coarse stage) ----------------------------------
def central_any(s, vs, mode, mut=None):
    """[3, X, Y, Z]: the central differences of s [X, Y, Z]"""
    out = []
    for a in range(3):
        n = s.shape[a]
        p_ = pos(s.shape, a)
        interior = (p_ >= 1) & (p_ <= n - 2)
        d = xhalf(_lift(nbr(s, a, 1), mode) - _lift(nbr(s, a, -1), mode)) / _c(vs, mode)
        if mut != "boundary_layer_one_sided":
            d = xwhere(interior, d, Q(torch.zeros(s.shape, dtype=F64)) if mode == "q" else torch.zeros(s.shape))
        out.append(d)
    return out


def central_adj_any(e, mode, mut=None):
    """sum_c [q - e_c interior] e_c[q - e_c] - [q + e_c interior] e_c[q + e_c], e a list of three [X, Y, Z]; in the kernel's order"""
    acc = None
    for a in range(3):
        n = e[a].shape[a]
        p_ = pos(e[a].shape, a)
        lo, hi = (p_ - 1 >= 1) & (p_ - 1 <= n - 2), (p_ + 1 >= 1) & (p_ + 1 <= n - 2)
        if mut == "adjoint_collects_boundary_sources":
            lo, hi = p_ - 1 >= 0, p_ + 1 <= n - 1
        zero = Q(torch.zeros(e[a].shape, dtype=F64)) if mode == "q" else torch.zeros(e[a].shape)
        tl, th = xwhere(lo, _lift(nbr(e[a], a, -1), mode), zero), xwhere(hi, _lift(nbr(e[a], a, 1), mode), zero)
        acc = tl - th if acc is None else (acc + tl) - th
    return acc


def _stack_q(qs):
    return (torch.stack([q.v.detach() for q in qs]), torch.stack([q.E for q in qs]), None)


# ---- smoothed-gradient TV term ----------------------------------------------------------------------------------------
MASKS = ("empty", "full", "corner cell", "interior cell", "random 50 %")
SMOOTH_CASES = {f"{g}_{m.split()[0]}": (g, m, "random") for g in SMALL_GRIDS for m in ("full", "random 50 %")}
SMOOTH_CASES.update({f"{g}_{m.split()[0]}": (g, m, "random") for g in ("3x3x3", "5x4x3", "9x7x6") for m in ("empty", "corner cell", "interior cell")})
SMOOTH_CASES["1x1x7_empty"] = ("1x1x7", "empty", "random")
SMOOTH_CASES["9x7x6_symmetric"] = ("9x7x6", "random 50 %", "product")
SMOOTH_CASES[f"{BIG_GRID}_random"] = (BIG_GRID, "random 50 %", "random")


def _asym_weights(k, g_, scale):
    while True:
        w = torch.randn(k, k, k, generator=g_) * scale
        if torch.unique(w).numel() == w.numel() and bool((w > 0).any()) and bool((w < 0).any()):
            return w


def case_smooth(name):
    if ("smooth", name) in _CACHE:
        return _CACHE[("smooth", name)]
    gname, mk, wk = SMOOTH_CASES[name]
    dims = GRIDS[gname]
    g_ = _gen(5000 + sum(map(ord, name)))
    sdf = torch.randn(*dims, generator=g_)
    n = sdf.numel()
    census = grid_census(dims)
    if wk == "random":
        w, bias = _asym_weights(3, g_, 0.2), f32(0.3)
        census.add("asymmetric weights, non-zero bias")
    else:
        o = torch.tensor([1.0, 2.0, 1.0], dtype=F64)
        w, bias = ((o[:, None, None] * o[None, :, None] * o[None, None, :]) / 64).float(), 0.0
        census.add("the product's symmetric kernel")
    mask = torch.zeros(dims, dtype=torch.uint8)
    if mk == "full":
        mask[:] = 1
    elif mk == "corner cell":
        mask[-1, 0, -1] = 1
    elif mk == "interior cell":
        mask[dims[0] // 2, dims[1] // 2, dims[2] // 2] = 1
        assert "interior" in census
    elif mk == "random 50 %":
        mask = (torch.rand(*dims, generator=g_) < 0.5).to(torch.uint8) * 3      # (any non-zero byte selects)
    census.add(f"mask: {mk}")
    mc = int((mask != 0).sum())
    if mc == 0:
        census.add("masked_cells = 0")
    inp = dict(name=name, dims=dims, sdf=sdf, mask=mask, w=w, bias=bias, voxel=f32(0.0137), weight=f32(0.7), mc=mc, loss0=f32(1.25),
               work6=torch.randn(6, *dims, generator=g_), grad0=torch.randn(*dims, generator=g_) * 0.1, grad_out=torch.tensor([f32(1.7)]))
    inp["census"], inp["claims"] = census, set(census)
    _CACHE[("smooth", name)] = inp
    return inp


def _inv_count(inp, mut=None):
    """weight / (3.0f * (float)masked_cells) as the entry forms it, in binary32"""
    cells = inp["sdf"].numel() if mut == "mean_over_all_cells" else inp["mc"]
    return float(t32(inp["weight"]) / (t32(3.0) * t32(float(cells)))) if cells > 0 else 0.0


def _bwd_coeff(inp, with_go, mut=None):
    cells = inp["sdf"].numel() if mut == "mean_over_all_cells" else inp["mc"]
    c = t32(-2.0) * t32(inp["weight"]) / (t32(3.0) * t32(float(cells))) / t32(2.0) / t32(inp["voxel"])
    if with_go:
        c = c * inp["grad_out"][0]
    return -float(c) if mut == "backward_sign_swapped" else float(c)


def _loss_shape(n):
    blocks = min((n + 255) // 256, THREADS // 256)
    return blocks, -(-n // (blocks * 256))


def emu_smooth_fwd(inp, mut=None):
    g = torch.stack(central_any(inp["sdf"], inp["voxel"], "32", mut))
    s = corr3(g, _wmut(inp["w"], mut), 1) + t32(inp["bias"])
    e = s - g
    if mut != "mask_ignored_in_the_loss":
        e = torch.where((inp["mask"] != 0)[None], e, torch.zeros(()))
    loss = t32(inp["loss0"]) + (e * e).sum() * t32(_inv_count(inp, mut))
    return {"work6": torch.cat([g, e]), "loss": loss.reshape(1)}


def verify_smooth_fwd(inp, got, K):
    dims, n = inp["dims"], inp["sdf"].numel()
    gq = central_any(inp["sdf"], inp["voxel"], "q")
    g32 = torch.stack(central_any(inp["sdf"], inp["voxel"], "32"))      # exact inputs of pass 2 (asserted bit for bit below)
    m = (inp["mask"] != 0)[None].expand(3, *dims)
    gd, w = g32.double(), inp["w"].double()
    s = corr3(gd, w, 1) + inp["bias"]
    M = corr3(gd.abs(), w.abs(), 1) + abs(inp["bias"])
    e = torch.where(m, s - gd, torch.zeros((), dtype=F64))
    Ee = torch.where(m, 28 * M + e.abs(), torch.zeros((), dtype=F64))
    gv, gE, _ = _stack_q(gq)
    inv = _inv_count(inp)
    blocks, trips = _loss_shape(n)
    sq = float((e * e).sum())
    total = inv * sq
    loss_abs = inv * (float((2 * e.abs() * Ee + e * e).sum()) + (3 * trips + 9) * sq) + blocks * (abs(inp["loss0"]) + total)
    out = {"work6": (torch.cat([gv, e]), torch.cat([gE, Ee]), torch.cat([torch.zeros_like(m), ~m])),
           "loss": (torch.tensor([inp["loss0"] + total], dtype=F64), torch.tensor([loss_abs], dtype=F64), None)}
    six = torch.cat([torch.ones_like(m), torch.zeros_like(m)])
    b = {"work6": (six, torch.cat([g32, torch.zeros_like(g32)]))}
    if inp["mc"] == 0:
        b["loss"] = (torch.ones(1, dtype=torch.bool), torch.tensor([inp["loss0"]]))
    r = _ref(out, b)
    return (r,) + _judge(r, got, K)


def _smooth_bwd_any(inp, with_go, mode, mut=None):
    g0 = _lift(inp["grad0"], mode)
    cells = inp["sdf"].numel() if mut == "mean_over_all_cells" else inp["mc"]
    if cells == 0:
        return g0
    acc = central_adj_any(list(inp["work6"][3:]), mode, mut)
    return g0 + acc * _c(_bwd_coeff(inp, with_go, mut), mode)


def emu_smooth_bwd(inp, mut=None):
    return {"grad_sdf": _smooth_bwd_any(inp, True, "32", mut), "grad_sdf_null": _smooth_bwd_any(inp, False, "32", mut)}


def verify_smooth_bwd(inp, got, K):
    out = {"grad_sdf": _out(_smooth_bwd_any(inp, True, "q")), "grad_sdf_null": _out(_smooth_bwd_any(inp, False, "q"))}
    b = {}
    if inp["mc"] == 0:
        b = {k: (torch.ones(inp["dims"], dtype=torch.bool), inp["grad0"]) for k in out}
    r = _ref(out, b)
    return (r,) + _judge(r, got, K)


# ---- dense operators of the coarse stage ------------------------------------------------------------------------------
KS = (1, 3, 5, 7)
GAUSS_CASES = {f"{g}_k{k}": (g, k, "random") for g in GRIDS for k in KS if not (g == BIG_GRID and k == 7)}
GAUSS_CASES["9x7x6_k5_gaussian"] = ("9x7x6", 5, "product")


def case_gauss(name):
    if ("gauss", name) in _CACHE:
        return _CACHE[("gauss", name)]
    gname, k, wk = GAUSS_CASES[name]
    dims = GRIDS[gname]
    g_ = _gen(6000 + sum(map(ord, name)))
    census = grid_census(dims) | {f"k = {k}"}
    if wk == "random":
        w = _asym_weights(k, g_, 1.0 / k) if k > 1 else torch.tensor([[[f32(-0.7)]]])
        census.add("asymmetric weights")
    else:
        from oracle.coarse_path import gaussian_kernel
        w = gaussian_kernel(k, 1.0)[0, 0].float()
        census.add("the product's symmetric kernel")
    if all(d < k // 2 for d in dims):
        census.add("every axis shorter than r")
    inp = dict(name=name, dims=dims, k=k, w=w, x=torch.randn(*dims, generator=g_), gout=torch.randn(*dims, generator=g_),
               gin0=torch.randn(*dims, generator=g_) * 0.5)
    inp["census"], inp["claims"] = census, set(census)
    _CACHE[("gauss", name)] = inp
    return inp


def emu_gauss_fwd(inp, mut=None):
    return {"out": corr3(inp["x"], _wmut(inp["w"], mut), inp["k"] // 2)}


def verify_gauss_fwd(inp, got, K):
    k, x, w = inp["k"], inp["x"].double(), inp["w"].double()
    val, M = corr3(x, w, k // 2), corr3(x.abs(), w.abs(), k // 2)
    r = _ref({"out": (val, (k ** 3 + 1) * M, None)})
    return (r,) + _judge(r, got, K)


def _adjoint(gout, w, r):
    x = torch.zeros_like(gout, requires_grad=True)
    (g,) = torch.autograd.grad((corr3(x, w, r) * gout).sum(), x)
    return g


def _gauss_bwd_scatter32(inp, mut):
    """the adjoint as a scatter over the taps, in binary32: gin[clamp(o + t - r)] += w[t] gout[o]"""
    k, dims, w = inp["k"], inp["dims"], _wmut(inp["w"], mut)
    r = k // 2
    if mut == "adjoint_kernel_flipped_on_one_axis":
        w = w.flip(2)
    acc = torch.zeros(inp["gout"].numel())
    o = [pos(dims, a).reshape(-1) for a in range(3)]
    for a in range(k):
        for b in range(k):
            for c in range(k):
                t = [(o[0] + a - r).clamp(0, dims[0] - 1), (o[1] + b - r).clamp(0, dims[1] - 1), (o[2] + c - r).clamp(0, dims[2] - 1)]
                keep = torch.ones_like(t[0], dtype=torch.bool)
                if mut == "tap_range_one_short_at_upper_face" and dims[0] > 1:
                    keep = ~((t[0] == dims[0] - 1) & (a == 2 * r))
                i = (t[0] * dims[1] + t[1]) * dims[2] + t[2]
                acc.index_add_(0, i[keep], (w[a, b, c] * inp["gout"].reshape(-1))[keep])
    return inp["gin0"] + acc.reshape(dims)


def emu_gauss_bwd(inp, mut=None):
    if mut is None:
        return {"gin": inp["gin0"] + _adjoint(inp["gout"], inp["w"], inp["k"] // 2)}
    return {"gin": _gauss_bwd_scatter32(inp, mut)}


def verify_gauss_bwd(inp, got, K):
    k, go, w = inp["k"], inp["gout"].double(), inp["w"].double()
    val = inp["gin0"].double() + _adjoint(go, w, k // 2)
    M = _adjoint(go.abs(), w.abs(), k // 2)
    r = _ref({"gin": (val, (k ** 3 + 2) * M + val.abs(), None)})
    return (r,) + _judge(r, got, K)


CENTRAL_CASES = {g: g for g in GRIDS}


def case_central(name):
    if ("central", name) in _CACHE:
        return _CACHE[("central", name)]
    dims = GRIDS[name]
    g_ = _gen(7000 + sum(map(ord, name)))
    inp = dict(name=name, dims=dims, sdf=torch.randn(*dims, generator=g_), voxel=f32(0.0213), g=torch.randn(*dims, 3, generator=g_),
               gsdf0=torch.randn(*dims, generator=g_) * 10)
    inp["census"] = grid_census(dims)
    inp["claims"] = set(inp["census"])
    _CACHE[("central", name)] = inp
    return inp


def emu_central_fwd(inp, mut=None):
    return {"grad": torch.stack(central_any(inp["sdf"], inp["voxel"], "32", mut), -1)}


def verify_central_fwd(inp, got, K):
    v, E, _ = _stack_q(central_any(inp["sdf"], inp["voxel"], "q"))
    r = _ref({"grad": (v.permute(1, 2, 3, 0), E.permute(1, 2, 3, 0), None)})
    return (r,) + _judge(r, got, K)


def _central_bwd_any(inp, mode, mut=None):
    acc = central_adj_any([inp["g"][..., c] for c in range(3)], mode, mut)
    if mut == "backward_sign_swapped":
        acc = -acc
    return _lift(inp["gsdf0"], mode) + xhalf(acc) / _c(inp["voxel"], mode)


def emu_central_bwd(inp, mut=None):
    return {"gsdf": _central_bwd_any(inp, "32", mut)}


def verify_central_bwd(inp, got, K):
    r = _ref({"gsdf": _out(_central_bwd_any(inp, "q"))})
    return (r,) + _judge(r, got, K)


# =======================================================================================================================
# the comparison, the operations, their families and the mutants
# =======================================================================================================================
def _judge(r, got, K):
    """shade_ref64.compare plus the bit expectations of Ref.bits"""
    worst, fails = compare(r, {k: got[k] for k in r.out if k in got}, K)
    for name, (mask, want) in r.bits.items():
        if name not in got:
            fails.append(f"{name}: missing")
            continue
        g = got[name].detach().cpu().reshape(want.shape)
        g = g.to(want.dtype) if want.dtype != F32 else g.float()
        bad = (bits(g) != bits(want)) & mask
        if bool(bad.any()):
            i = int(torch.nonzero(bad.reshape(-1))[0])
            fails.append(f"{name}: {int(bad.sum())} of {int(mask.sum())} values differ in their bits; first at flat index {i}: got "
                         f"{float(g.reshape(-1)[i])!r}, want {float(want.reshape(-1)[i])!r}")
    return worst, fails


# op -> (case builder, case names, verify(inp, got, K) -> (ref, worst, fails), binary32 emulation, family, C entry points)
OPS = {
    "adam_step": (case_adam, list(ADAM_CASES), verify_adam, emu_adam, "adam", ("esr_adam_step",)),
    "adam_live": (case_live, list(LIVE_CASES), verify_adam_live, emu_adam_live, "adam", ("esr_adam_step_live",)),
    "live_from_moments": (case_from_moments, LIVE_NS, verify_from_moments, emu_from_moments, "adam", ("esr_brick_live_from_moments",)),
    "tv_add_grad": (case_tv, list(TV_CASES), verify_tv, emu_tv, "tv_add_grad", ("esr_tv_add_grad",)),
    "smooth_tv_fwd": (case_smooth, list(SMOOTH_CASES), verify_smooth_fwd, emu_smooth_fwd, "smooth_tv", ("esr_smooth_grad_tv_fwd",)),
    "smooth_tv_bwd": (case_smooth, list(SMOOTH_CASES), verify_smooth_bwd, emu_smooth_bwd, "smooth_tv", ("esr_smooth_grad_tv_bwd",)),
    "gauss3d_fwd": (case_gauss, list(GAUSS_CASES), verify_gauss_fwd, emu_gauss_fwd, "gauss", ("esr_gauss3d_fwd",)),
    "gauss3d_bwd": (case_gauss, list(GAUSS_CASES), verify_gauss_bwd, emu_gauss_bwd, "gauss", ("esr_gauss3d_bwd",)),
    "central_grad_fwd": (case_central, list(CENTRAL_CASES), verify_central_fwd, emu_central_fwd, "central", ("esr_central_grad_fwd",)),
    "central_grad_bwd": (case_central, list(CENTRAL_CASES), verify_central_bwd, emu_central_bwd, "central", ("esr_central_grad_bwd",)),
}


def build(op, case):
    return OPS[op][0](case)


def all_cases():
    return [(op, case) for op, spec in OPS.items() for case in spec[1]]


def is_big(case):
    return str(case) in (ADAM_BIG, "big") or str(case).startswith(BIG_GRID)


def verify(op, inp, got, K):
    r, worst, fails = OPS[op][2](inp, dict(got), K)
    r.flips, r.share = {}, 0.0                                         # no operation here has a banded decision
    return r, worst, fails


# K per family, for both test files: the next power of two at or above twice the worst ratio |gpu - ref| / (U absref) measured on the
# MI355X over every case of test_gpu_grid_ref64.py (printed under -s); the factor two leaves room for the order of the float atomics
# of `loss`.  The binary32 emulation reaches the same worst ratios to three digits (they seeded the constants before the GPU run), and
# of the 630 values with a subnormal intermediate (adam, gradients down to 1e-20) the device flushed none.
K_FAMILY = {
    "adam": 2,          # measured worst 0.992 (esr_adam_step and esr_adam_step_live; esr_brick_live_from_moments is exact)
    "tv_add_grad": 2,   # 0.888 (esr_tv_add_grad, dense and sparse)
    "smooth_tv": 2,     # 0.998 (esr_smooth_grad_tv_fwd: the gradient field; esr_smooth_grad_tv_bwd 0.998)
    "gauss": 2,         # 0.988 (esr_gauss3d_bwd at k = 1; esr_gauss3d_fwd 0.457)
    "central": 2,       # 1.000 (esr_central_grad_fwd; esr_central_grad_bwd 0.953)
}

# mutant of the emulation -> the ops it applies to; each must break the bound (or a bit expectation) on at least one small case of
# each of those ops
MUTANTS = {
    "adjoint_kernel_flipped_on_one_axis": ["gauss3d_bwd"],
    "conv_taps_transposed_xz": ["gauss3d_fwd", "gauss3d_bwd", "smooth_tv_fwd"],
    "tap_range_one_short_at_upper_face": ["gauss3d_bwd"],
    "boundary_layer_one_sided": ["smooth_tv_fwd", "central_grad_fwd"],
    "adjoint_collects_boundary_sources": ["smooth_tv_bwd", "central_grad_bwd"],
    "backward_sign_swapped": ["smooth_tv_bwd", "central_grad_bwd"],
    "clamp_dropped": ["tv_add_grad"],
    "wy_on_i_axis": ["tv_add_grad"],
    "seam_neighbour_read": ["tv_add_grad"],
    "sparse_updates_zero_gradient_cells": ["tv_add_grad"],
    "mask_ignored_in_the_loss": ["smooth_tv_fwd"],
    "mean_over_all_cells": ["smooth_tv_fwd", "smooth_tv_bwd"],
    "bias_correction_with_step_minus_1": ["adam_step"],
    "eps_inside_sqrt": ["adam_step"],
    "per_lr_on_denominator": ["adam_step"],
    "weight_decay_after_moments": ["adam_step"],
    "float4_w_takes_z_per_lr": ["adam_step"],
    "scalar_tail_skipped": ["adam_step"],
    "live_brick_with_zero_gradient_skipped": ["adam_live"],
    "ragged_brick_dropped": ["adam_live", "live_from_moments"],
    "gradient_zeroed_in_dead_brick": ["adam_live"],
}
