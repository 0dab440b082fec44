"""CPU checks of the poison harness (tests/poison.py): the allocation hooks, the walker, ``compare``, three toy "steps" that
show which leg catches which kind of dependence, and the SCRATCH / STATE table against the engine classes' sources."""
import ast
import inspect
import os
import re

import pytest
import torch

import poison
from poison import LEGS, SCRATCH, STATE, Entry, compare, poisoned_allocations, repoison

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERYWHERE = lambda t: True                    # the hooks' device filter, so that they can be exercised on CPU tensors
HERE = (__name__,)                             # the walker descends into this module's fake classes


# ---- the hooks -----------------------------------------------------------------------------------------------------------
def _originals():
    return torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__


def test_hooks_fill_count_and_restore():
    before = _originals()
    with poisoned_allocations(poison.NAN, 0, device_filter=EVERYWHERE) as pa:
        assert torch.empty is not before[0] and torch.Tensor.new_empty is not before[3]
        a = torch.empty(7, 3)
        b = torch.empty_like(a, dtype=torch.int64)
        c = torch.empty_strided((4, 5), (1, 4), dtype=torch.float16)
        d = a.new_empty((2, 2), dtype=torch.bool)
        e = torch.empty(0)                                            # nothing to fill: not counted
        assert bool(torch.isnan(a).all()) and int(b.abs().sum()) == 0 and bool(torch.isnan(c).all()) and not bool(d.any())
        assert c.stride() == (1, 4) and e.numel() == 0
        assert pa.allocations == 4 and pa.bytes == 7 * 3 * 4 + 21 * 8 + 20 * 2 + 4
    after = _originals()
    assert all(x is y for x, y in zip(before[:4], after[:4])) and before[4] == after[4]
    with pytest.raises(ZeroDivisionError):
        with poisoned_allocations(0.0, 0, device_filter=EVERYWHERE):
            torch.empty(3)
            1 / 0
    after = _originals()
    assert all(x is y for x, y in zip(before[:4], after[:4])) and before[4] == after[4]


def test_default_filter_leaves_host_tensors_alone():
    with poisoned_allocations(poison.NAN, 1) as pa:
        x = torch.empty(1000, dtype=torch.int32)
        y = torch.empty(16)
    assert pa.allocations == 0 and pa.bytes == 0 and x.numel() == 1000 and y.numel() == 16


@pytest.mark.parametrize("dtype,itype,bits", [(torch.float32, torch.int32, 0x7FC00000), (torch.float16, torch.int16, 0x7E00),
                                              (torch.bfloat16, torch.int16, 0x7FC0),
                                              (torch.float64, torch.int64, 0x7FF8000000000000)])
def test_nan_bit_patterns_and_leg_c_values(dtype, itype, bits):
    with poisoned_allocations(*LEGS["B"], device_filter=EVERYWHERE):
        t = torch.empty(33, dtype=dtype)
    assert torch.equal(t.view(itype), torch.full((33,), bits, dtype=itype))
    with poisoned_allocations(*LEGS["C"], device_filter=EVERYWHERE):
        t = torch.empty(33, dtype=dtype)
        i = torch.empty(5, dtype=torch.uint8)
    want = 60000.0 if dtype == torch.float16 else 2.0 ** 100
    assert torch.equal(t.double(), torch.full((33,), want, dtype=torch.float64)) and i.tolist() == [1] * 5
    with poisoned_allocations(*LEGS["A"], device_filter=EVERYWHERE):
        t = torch.empty(33, dtype=dtype)
    assert int(torch.count_nonzero(t)) == 0 and not bool(torch.signbit(t).any())


def test_march_cache_rows_and_byte_buffers():
    cap, rays = 64, 3
    t = torch.zeros(rays * 5 * cap)
    poison.fill_march_cache(t, cap, poison.NAN, 1)
    v = t.view(rays, 5, cap)
    assert bool(torch.isnan(v[:, [0, 2, 3]]).all())
    assert torch.equal(v.view(torch.int32)[:, [1, 4]], torch.ones(rays, 2, cap, dtype=torch.int32))      # valid step / info words
    with pytest.raises(ValueError):
        poison.fill_march_cache(torch.zeros(7), cap, 0.0, 0)
    x16 = torch.zeros(64, dtype=torch.uint8)
    poison.fill_as_bf16(x16, poison.NAN, 1)
    assert torch.equal(x16.view(torch.int16), torch.full((32,), 0x7FC0, dtype=torch.int16))


# ---- the walker on a small fake engine -----------------------------------------------------------------------------------
class _FakeWorkspace:
    def __init__(self):
        self.buf = {k: torch.arange(64, dtype=torch.float32) for k in ("X", "H0")}
        self.buf["rec_ray"] = torch.arange(32, dtype=torch.int32)
        self.ray_bufs = {512: dict(cnt3=torch.arange(8, dtype=torch.int32))}
        self.cache = None

    def __getitem__(self, k):
        if k not in self.buf and k == "dXt":                          # a lazy buffer: allocated by its first reader
            self.buf[k] = torch.arange(16, dtype=torch.float32)
        return self.buf[k]


class _FakeEngine:
    def __init__(self):
        self.ws = _FakeWorkspace()
        self.packed = dict(off=torch.arange(10, dtype=torch.float32), emo=torch.arange(10, dtype=torch.float32) - 3)
        self.plan_dev = torch.arange(8, dtype=torch.int32)
        self.passes = [dict(scratch=[torch.ones(5), (torch.ones(6),)])]
        self.twice = self.ws.buf["X"]                                  # the same tensor under a second name
        self.window = self.ws.buf["X"][8:24]                           # ... and a view of its storage
        self.host_word = 3
        self.name = "fake"


FAKE_TABLE = {
    ("_FakeWorkspace", "buf"): Entry(None, names=((r"X|H0|dXt|rec_ray", SCRATCH, "toy"),)),
    ("_FakeWorkspace", "ray_bufs"): Entry(SCRATCH, "toy"),
    ("_FakeEngine", "packed"): Entry(STATE, "toy"),
    ("_FakeEngine", "plan_dev"): Entry(STATE, "toy"),
    ("_FakeEngine", "passes"): Entry(SCRATCH, "toy"),
    ("_FakeEngine", "twice"): Entry(SCRATCH, "toy", how="alias"),
    ("_FakeEngine", "window"): Entry(SCRATCH, "toy", how="alias"),
}


def _walk(eng, leg="B", table=FAKE_TABLE):
    return repoison(eng, *LEGS[leg], table=table, device_filter=EVERYWHERE, descend_modules=HERE)


def test_walker_fills_scratch_leaves_state_and_visits_each_storage_once():
    eng = _FakeEngine()
    state = {k: v.clone() for k, v in eng.packed.items()}
    plan = eng.plan_dev.clone()
    rep = _walk(eng)
    # X (reached three times: once), H0, rec_ray, cnt3, the two nested scratch tensors | packed x 2, plan_dev
    assert (rep.storages, rep.filled, rep.state) == (9, 6, 3)
    assert rep.bytes == (64 + 64 + 32 + 8 + 5 + 6) * 4
    assert len({p for p, _ in rep.names}) == 6
    assert bool(torch.isnan(eng.ws.buf["X"]).all()) and bool(torch.isnan(eng.ws.buf["H0"]).all())
    assert int(eng.ws.buf["rec_ray"].abs().sum()) == 0 and int(eng.ws.ray_bufs[512]["cnt3"].abs().sum()) == 0
    assert bool(torch.isnan(eng.passes[0]["scratch"][0]).all()) and bool(torch.isnan(eng.passes[0]["scratch"][1][0]).all())
    for k, v in state.items():
        assert torch.equal(eng.packed[k], v)                           # bit-identical
    assert torch.equal(eng.plan_dev, plan)
    # the lazy buffer exists only after its first reader asked for it
    eng.ws["dXt"]
    rep2 = _walk(eng, "C")
    assert rep2.storages == 10 and rep2.filled == 7
    assert float(eng.ws.buf["dXt"][3]) == 2.0 ** 100 and int(eng.ws.buf["rec_ray"][5]) == 1
    # a storage that any STATE tensor shares is left alone, whatever else points into it
    eng.passes.append(dict(scratch=[eng.packed["off"][2:5]]))
    _walk(eng, "B")
    assert torch.equal(eng.packed["off"], state["off"])


def test_walker_fails_on_an_unclassified_tensor():
    eng = _FakeEngine()
    eng.mystery = torch.zeros(4)
    with pytest.raises(poison.Unclassified, match="mystery"):
        _walk(eng)
    eng = _FakeEngine()
    eng.ws.buf["new_buffer"] = torch.zeros(4)                          # a workspace name the table does not know
    with pytest.raises(poison.Unclassified, match="new_buffer"):
        _walk(eng)
    assert bool((eng.ws.buf["X"] == torch.arange(64)).all())           # nothing was filled before the failure


class _FakeOpt:
    def __init__(self):
        self._zeroed = set()


class _FakeStep:
    def __init__(self):
        self._flat = torch.ones(100)
        self._views = ("key", self._flat, dict(a=self._flat[:40], b=self._flat[40:70], w=self._flat[70:]))
        self.zero_fill_by = None
        self.model = torch.nn.Linear(6, 5)
        self.model.weight.grad = self._flat[70:].view(5, 6)           # what _Step.assign_grads does
        self.model.bias.grad = torch.full((5,), 7.0)                  # a gradient of autograd's own: not ours to fill


def test_flat_gradient_buffer_keeps_the_ranges_the_live_optimizer_marked():
    table = {("_FakeStep", "_flat"): poison.TABLE[("_Step", "_flat")], ("_FakeStep", "_views"): poison.TABLE[("_Step", "_views")]}
    table.update({k: v for k, v in poison.TABLE.items() if k[0] == "Module"})
    st = _FakeStep()
    w, b = st.model.weight.detach().clone(), st.model.bias.detach().clone()
    rep = repoison(st, *LEGS["B"], table=table, device_filter=EVERYWHERE, descend_modules=HERE)
    # param.grad views of the buffer do not shield it; parameters are STATE; a gradient that aliases nothing we own stays
    assert rep.filled == 1 and bool(torch.isnan(st._flat).all()) and bool(torch.isnan(st.model.weight.grad).all())
    assert torch.equal(st.model.weight.detach(), w) and torch.equal(st.model.bias.detach(), b)
    assert torch.equal(st.model.bias.grad, torch.full((5,), 7.0))
    st = _FakeStep()
    st._flat.zero_()
    st.zero_fill_by = _FakeOpt()
    b = st._views[2]["b"]
    st.zero_fill_by._zeroed.add((b.device, b.data_ptr(), b.numel()))   # optimizer._mem_key of a grid the live kernel zeroed
    repoison(st, *LEGS["B"], table=table, device_filter=EVERYWHERE, descend_modules=HERE)
    assert bool(torch.isnan(st._flat[:40]).all()) and bool(torch.isnan(st._flat[70:]).all())
    assert int(torch.count_nonzero(st._flat[40:70])) == 0


# ---- teeth: which leg catches which dependence ---------------------------------------------------------------------------
ROWS = 2


class _ToyWorkspace:
    """Grow-only, tile-major [tiles][ROWS][32], with headroom: the shape of fine_engine._Workspace."""

    def __init__(self):
        self.cap, self.buf = 0, None

    def ensure(self, tiles):
        if tiles > self.cap:
            self.cap = int(tiles * 1.25) + 2
            self.buf = torch.empty(self.cap * ROWS * 32, dtype=torch.float32)


TOY_TABLE = {("_ToyWorkspace", "buf"): Entry(SCRATCH, "producer writes the live lanes of tiles [0, tiles) -> the reduction of the same step")}


def _fmax_reduce(v):
    """A reduction by fmaxf: a NaN operand is ignored."""
    return torch.nan_to_num(v, nan=float("-inf")).max()


def _toy_step(ws, x, variant):
    n = x.numel()
    tiles = (n + 31) // 32
    ws.ensure(tiles)
    v = ws.buf[: tiles * ROWS * 32].view(tiles, ROWS, 32)
    live = (torch.arange(tiles * 32) < n).view(tiles, 32)
    xs = torch.zeros(tiles * 32)
    xs[:n] = x
    v[:, 0, :][live] = xs.view(tiles, 32)[live]                        # the producer writes live lanes only
    if variant == "sums_padding_lanes":                                # a 32-lane sum over whole tiles
        return v[:, 0, :].sum(), _fmax_reduce(torch.where(live, v[:, 0, :], torch.zeros(())))
    if variant == "max_over_stale_tail":                               # an fmax over the capacity, not the step's live lanes
        return torch.where(live, v[:, 0, :], torch.zeros(())).sum(), _fmax_reduce(ws.buf.view(ws.cap, ROWS, 32)[:, 0, :])
    assert variant == "masked"
    return torch.where(live, v[:, 0, :], torch.zeros(())).sum(), _fmax_reduce(torch.where(live, v[:, 0, :], torch.zeros(())))


def _toy_run(variant, leg):
    g = torch.Generator().manual_seed(5)
    xs = [torch.rand(n, generator=g) + 0.5 for n in (70, 37, 70)]       # ragged, fewer tiles than before, back up
    out = {}
    with poisoned_allocations(*LEGS[leg], device_filter=EVERYWHERE) as pa:
        ws = _ToyWorkspace()
        for i, x in enumerate(xs):
            if ws.buf is not None:
                repoison(ws, *LEGS[leg], table=TOY_TABLE, device_filter=EVERYWHERE, descend_modules=HERE)
            s, m = _toy_step(ws, x, variant)
            out[f"step{i}"] = dict(sum=s.clone(), max=m.clone())
        assert pa.bytes > 0 and any(x.numel() % 32 for x in xs) and (37 + 31) // 32 < ws.cap
    return out


def _caught(variant, leg):
    try:
        compare(_toy_run(variant, "A"), _toy_run(variant, leg), deterministic=("step0", "step1", "step2"))
    except poison.Mismatch:
        return True
    return False


def test_teeth_each_leg_catches_what_it_is_there_for():
    assert _caught("sums_padding_lanes", "B")                          # NaN reaches the 32-lane sum
    assert _caught("sums_padding_lanes", "C")
    assert not _caught("max_over_stale_tail", "B")                     # fmax ignores NaN: leg B is blind here ...
    assert _caught("max_over_stale_tail", "C")                         # ... and 2^100 is not
    assert not _caught("masked", "B") and not _caught("masked", "C")   # the correct step passes every leg


# ---- compare on planted differences -------------------------------------------------------------------------------------
def _results():
    g = torch.Generator().manual_seed(1)
    return dict(loss=0.25, grads=dict(w=torch.randn(50, generator=g), b=torch.randn(7, generator=g)),
                out=torch.randn(9, 3, generator=g), idx=torch.arange(6), counts=dict(m0=5, m3=17), fallbacks=0)


def _clone(r):
    return {k: ({kk: (vv.clone() if torch.is_tensor(vv) else vv) for kk, vv in v.items()} if isinstance(v, dict)
                else v.clone() if torch.is_tensor(v) else v) for k, v in r.items()}


def test_compare_accepts_the_twin_and_rejects_planted_differences():
    a = _results()
    a["grads"]["w"][0] = 4.0                                           # max |w| = 4: the scale of rel_err
    errs = compare(a, _clone(a), deterministic=("out",))
    assert set(errs) == {"loss", "grads/w", "grads/b"} and max(errs.values()) == 0.0

    def planted(edit, **kw):
        b = _clone(a)
        edit(b)
        try:
            compare(a, b, deterministic=("out",), **kw)
        except poison.Mismatch as e:
            return str(e)
        return None

    assert "non-finite" in planted(lambda b: b["grads"]["w"].__setitem__(3, float("nan")))
    assert "non-finite" in planted(lambda b: b["out"].__setitem__((2, 1), float("inf")))
    assert "counts/m3" in planted(lambda b: b["counts"].__setitem__("m3", 18))
    assert "fallbacks" in planted(lambda b: b.__setitem__("fallbacks", 1))
    assert "idx" in planted(lambda b: b["idx"].__setitem__(2, 9))

    def flip_sign(b):
        b["out"][4, 0] = 0.0
    a["out"][4, 0] = -0.0                                              # -0.0 == 0.0: only the sign bit differs
    assert "deterministic" in planted(flip_sign)

    def nudge(rel):
        def edit(b):
            b["grads"]["w"] = (b["grads"]["w"].double() + torch.nn.functional.one_hot(torch.tensor(7), 50) * rel * 4.0)
        return edit
    a["grads"]["w"] = a["grads"]["w"].double()
    assert "grads/w" in planted(nudge(1.01e-5))                        # just over the bar of the fine step
    assert planted(nudge(0.99e-5)) is None                             # just under it
    assert "grads/w" in planted(nudge(1.5e-5), bar=poison.BAR_FINE) and planted(nudge(1.5e-5), bar=poison.BAR_LTS) is None
    assert "deterministic" in planted(lambda b: b["out"].__setitem__((0, 0), float(b["out"][0, 0]) * (1 + 2e-7)))
    b = _clone(a)
    del b["loss"]
    with pytest.raises(poison.Mismatch, match="keys"):
        compare(a, b)


# ---- the table against the sources --------------------------------------------------------------------------------------
def _src(rel):
    with open(os.path.join(ROOT, "esr_nerf_amd", rel)) as f:
        return f.read()


def _dict_call_keys(tree, name):
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in node.targets):
            assert isinstance(node.value, ast.Call) and getattr(node.value.func, "id", None) == "dict", name
            assert all(k.arg is not None for k in node.value.keywords), f"{name}: a ** entry cannot be checked"
            return [k.arg for k in node.value.keywords]
    raise AssertionError(f"{name} not found")


def _matches(patterns, name):
    return any(re.fullmatch(p, name) for p, _, _ in patterns)


def test_fine_workspace_names_match_the_source():
    tree = ast.parse(_src("fine_engine.py"))
    names = _dict_call_keys(tree, "FINE_ROWS") + _dict_call_keys(tree, "FINE_OTHER")
    assert len(names) == len(set(names))
    assert set(names) == set(poison.FINE_BUFFERS), set(names) ^ set(poison.FINE_BUFFERS)
    # ... and the coarse engine's (built by a comprehension: read from the class)
    from esr_nerf_amd.fine_engine import FINE_OTHER, FINE_ROWS
    from esr_nerf_amd.voxurfc import CoarseEngine
    assert set(FINE_ROWS) | set(FINE_OTHER) == set(names)
    entry = poison.TABLE[("_Workspace", "buf")]
    for n in list(CoarseEngine.ROWS) + list(CoarseEngine.OTHER):
        assert _matches(entry.names, n), n
    assert not _matches(entry.names, "X17") and not _matches(entry.names, "off.H2")


def _sample_names(node):
    """The names a ``Pass.buf`` argument can take: a literal, or an f-string with its fields replaced by every net name /
    layer 0."""
    if isinstance(node, ast.Constant) and isinstance(node.value, str):
        return [node.value]
    if isinstance(node, ast.JoinedStr):
        outs = [""]
        for part in node.values:
            if isinstance(part, ast.Constant):
                outs = [o + part.value for o in outs]
            else:
                var = ast.unparse(part.value)
                subs = ["0", "2"] if var == "l" else ["off", "emo", "tone", "brdf", "emit"] if var in ("net", "nm") else None
                assert subs is not None, f"unknown f-string field {var}"
                outs = [o + s for o in outs for s in subs]
        return outs
    return None


def test_pass_buffer_names_match_the_call_sites():
    tree = ast.parse(_src("lts_engine.py"))
    pats = poison.PASS_BUFFERS
    parents = {}
    for node in ast.walk(tree):
        for ch in ast.iter_child_nodes(node):
            parents[ch] = node

    def enclosing(node):
        while node in parents:
            node = parents[node]
            if isinstance(node, ast.FunctionDef):
                return node.name
        return None

    seen, dynamic = set(), set()
    for node in ast.walk(tree):
        if not isinstance(node, ast.Call):
            continue
        f = node.func
        fname = f.attr if isinstance(f, ast.Attribute) else getattr(f, "id", None)
        args = []
        if fname == "buf" and node.args:
            args = [node.args[0]]
        elif fname == "_act" and len(node.args) >= 3:
            args = [node.args[2]]                                       # _act(P, zname, out, ...)
        elif fname == "from_rowmajor" and node.args:
            args = [node.args[0]]
        elif fname == "dict":
            args = [k.value for k in node.keywords if k.arg == "out"]   # the jobs of _act_batch
        for a in args:
            names = _sample_names(a)
            if names is None:
                assert fname == "buf", ast.unparse(node)
                dynamic.add(enclosing(node))
                continue
            for n in names:
                seen.add(n)
                assert _matches(pats, n), f"Pass buffer {n!r} ({ast.unparse(node)[:80]}) is not in poison.PASS_BUFFERS"
    # the call sites whose name is a variable get it from the callers checked above
    assert dynamic == {"from_rowmajor", "_act", "_act_batch"}, dynamic
    assert {"rec_ray", "X", "off.H0", "brdf.M2", "emit.a", "emo.ga", "pbr.t", "tone.dz"} <= seen
    assert not _matches(pats, "scratch") and not _matches(pats, "off.H")
    # every pattern is used by some call site
    for p, _, _ in pats:
        assert any(re.fullmatch(p, n) for n in seen), p


def _class_attrs(cls):
    """Attribute names a class's source assigns (``self.x = ``, class-level names, dataclass fields)."""
    tree = ast.parse(inspect.getsource(inspect.getmodule(cls)))
    out = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ClassDef) and node.name == cls.__name__:
            for sub in ast.walk(node):
                if isinstance(sub, ast.Attribute) and isinstance(sub.value, ast.Name) and sub.value.id in ("self", "eng") \
                        and isinstance(sub.ctx, ast.Store):
                    out.add(sub.attr)
                elif isinstance(sub, ast.AnnAssign) and isinstance(sub.target, ast.Name):
                    out.add(sub.target.id)
                elif isinstance(sub, ast.Assign):
                    out |= {t.id for t in sub.targets if isinstance(t, ast.Name)}
    return out | set(getattr(cls, "__slots__", ()))


def test_every_table_row_names_an_attribute_that_exists():
    from esr_nerf_amd import dvgo, esrnerf, fine_engine, lts_engine, modules, optimizer, trainer, voxurfc, voxurff
    classes = {c.__name__: c for c in (fine_engine._Workspace, fine_engine.March, fine_engine.FineEngine, lts_engine.Pass,
                                       lts_engine.LtsEngine, trainer._Step, optimizer.Adam, optimizer._Live, voxurff.VoxurfF,
                                       voxurfc.VoxurfC, dvgo.DVGO, modules.DenseGrid, modules.MaskCache)}
    generic = {"Module": {"_parameters", "_buffers", "grad"}, "Optimizer": {"state", "param_groups"}}
    for (owner, attr), entry in poison.TABLE.items():
        assert entry.cls in (SCRATCH, STATE) or entry.names, (owner, attr)
        assert entry.note or entry.names, (owner, attr)
        if owner in generic:
            assert attr in generic[owner], (owner, attr)
            continue
        assert owner in classes, f"table row for an unknown class {owner}"
        if attr == "*":
            attrs = _class_attrs(classes[owner])
            for pat, _, _ in entry.names:
                assert any(re.fullmatch(pat, a) for a in attrs), (owner, pat)
            continue
        have = set()
        for k in classes[owner].__mro__:
            if k.__module__.startswith("esr_nerf_amd"):
                have |= _class_attrs(k)
        assert attr in have, f"{owner}.{attr}: no such attribute in the source (renamed?)"
    # the buffers the issue names are where it says
    for key, cls in ((("_Workspace", "ray_bufs"), SCRATCH), (("_Workspace", "cache"), SCRATCH), (("FineEngine", "wgrad_scratch"), SCRATCH),
                     (("FineEngine", "tone_scratch"), SCRATCH), (("_Step", "_flat"), SCRATCH), (("FineEngine", "plan_dev"), STATE),
                     (("FineEngine", "range_flag"), STATE), (("FineEngine", "packed"), STATE), (("Optimizer", "state"), STATE),
                     (("_Live", "flags"), STATE)):
        assert poison.TABLE[key].cls == cls, key
    # the index-bearing allocation sites exist under the names the hook looks for
    src = _src("fine_engine.py")
    assert re.search(r"def _march_plan\(", src) and "need = int(L.esr_fine_march_cache_floats" in src and "ws.cache = torch.empty(need" in src
    assert re.search(r"def ensure\(self, tiles", src) and "for k, (per_tile, dtype) in self.other.items():" in src
    for site in poison.INDEX_SITES:
        assert {"module", "function", "what", "use", "treatment"} <= set(site)
