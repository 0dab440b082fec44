"""Poisoned uninitialised device memory: the harness of tests/test_poison_host.py and tests/test_gpu_poison.py (never
imported by the product).

The product allocates its workspaces with ``torch.empty`` and keeps them from step to step: grow-only, tile-major
(``[tiles][rows][32]``), sized with headroom.  A step with fewer tiles than the one before leaves whole stale tiles behind
its last one, a sample count that is no multiple of 32 leaves stale lanes inside the last tile, and rows above the ones a
kernel documents as written keep whatever was there.  The contract that none of this is ever READ lives in comments
("Uninitialised memory").  This module makes the stale content hostile and deterministic instead of "zeros or
small finite leftovers", so that a dependence shows up as a wrong number:

* ``poisoned_allocations(fpat, ival)`` -- a context manager that fills every tensor ``torch.empty`` / ``empty_like`` /
  ``empty_strided`` / ``Tensor.new_empty`` hands out on the device under test;
* ``repoison(obj, fpat, ival)`` -- a walker over everything reachable from an engine, step or optimizer object that fills
  every device tensor the table below classifies SCRATCH, leaves STATE alone and FAILS on a tensor in neither class;
* ``compare(a, b, deterministic, bar)`` -- the comparison of two legs' results.

Three legs per scenario (``LEGS``): A = zeros (the deterministic twin the others are compared with), B = quiet NaN (shows
anything multiplied or added in, ``0 * stale`` included), C = 2^100 / int 1 (shows what NaN hides: fmax / fmin /
compare-and-select, absmax-style reductions, conversions to fp16 planes that raise the range flag).

Index safety.  A latent bug must show up as a wrong number, never as a wild address, so a buffer whose VALUES a kernel turns
into an address, an offset or a trip count only ever gets values that are valid for that use (0 and 1):

* every integer / bool / uint8 buffer gets ``ival`` (0 or 1), whatever the leg -- that covers ``rec_ray`` (ray index:
  csrc/feat.hip:68, shade.hip:67, lts.hip:46 -- ``rays_o[3 * ray]``), ``rec_step`` (a step number that becomes a position, a
  float: feat.hip:72), ``cnt3`` / ``off3`` (record offsets: march.hip:220, :237), ``stats`` (``stats[3 r + 1]`` is the trip
  count of the cached fill and backward: march.hip:220, :239), the LTS passes' ``perm`` / ``inv_order`` / int64 ``rec_ray``
  (lts_engine._ref_order) and the ReLU mask words.  1 is a valid ray / step / offset because every poisoned scenario marches
  at least two rays of at least two steps each; the all-miss and the empty-batch steps launch no consumer of them;
* the march cache (``ws.cache``, fp32 ``[rays][5][cap]``) holds two INTEGER rows viewed through the float buffer: row 1
  (``step``, march.hip:226, :241) and row 4 (``info``: ``info >> 8`` is a record offset, march.hip:222, :355, :406).  Those
  two rows get ``ival`` as int32 bits, the float rows (sdf | alpha | T) get ``fpat`` (``fill_march_cache``; the allocation
  site is recognised by its caller, ``fine_engine.FineEngine._march_plan``, which also tells the row length ``cap``);
* ``X16`` is a uint8 buffer that holds bf16 operands: it is filled through a bf16 view with ``fpat`` (its bytes are data,
  never an index).

Float positions (``pts``, ray origins) need nothing: every grid fetch bounds-checks its corner indices
(esr_common.h: esr_tri_fetch1 / esr_ld_or0), so a NaN position reads zeros.
"""
from __future__ import annotations

import ctypes
import math
import re
import sys
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

import torch

SCRATCH, STATE = "scratch", "state"

NAN = float("nan")
BIG = 2.0 ** 100
# leg -> (fpat, ival)
LEGS = {"A": (0.0, 0), "B": (NAN, 0), "C": (BIG, 1)}

# the quiet NaN of each float type, as the integer type of the same width and its bits
NAN_BITS = {torch.float32: (torch.int32, 0x7FC00000), torch.float16: (torch.int16, 0x7E00),
            torch.bfloat16: (torch.int16, 0x7FC0), torch.float64: (torch.int64, 0x7FF8000000000000)}
FP16_BIG = 60000.0          # fp16 has no 2^100: the largest round value below its maximum (65504)

BAR_FINE = 1e-5             # two runs of the same fine / coarse step (tests/test_gpu_train_loop.py:163)
BAR_LTS = 2e-5              # two runs of the same LTS step (tests/test_gpu_lts_path.py:312)


def is_device_tensor(t: torch.Tensor) -> bool:
    """The default device filter: the GPU under test (CPU and pinned host tensors are left alone)."""
    return t.is_cuda


def fill(t: torch.Tensor, fpat: float, ival: int) -> None:
    """Fill ``t`` in place: floating types with ``fpat`` (NaN: the type's quiet-NaN bit pattern; fp16: +-60000 for what its
    range cannot hold), integer / bool / uint8 types with ``ival``."""
    if t.numel() == 0:
        return
    with torch.no_grad():
        t = t.detach()
        if t.is_floating_point():
            if fpat != fpat:
                it, bits = NAN_BITS[t.dtype]
                t.view(it).fill_(bits)
            else:
                v = float(fpat)
                if t.dtype == torch.float16 and abs(v) > FP16_BIG:
                    v = math.copysign(FP16_BIG, v)
                t.fill_(v)
        elif t.is_complex():
            raise TypeError("no poison pattern for complex tensors")
        elif t.dtype == torch.bool:
            t.fill_(bool(ival))
        else:
            t.fill_(int(ival))


MARCH_CACHE_ROWS = 5                    # csrc/march.hip: CACHE_ARR (sdf | step | alpha | T | info)
MARCH_CACHE_INT_ROWS = (1, 4)           # step, info: int32 viewed through the float buffer


def fill_march_cache(t: torch.Tensor, cap: int, fpat: float, ival: int) -> None:
    """The march cache ``[rays][5][cap]``: float rows with ``fpat``, the two integer rows with ``ival`` as int32 bits."""
    per_ray = MARCH_CACHE_ROWS * int(cap)
    if t.dtype != torch.float32 or cap <= 0 or t.numel() % per_ray:
        raise ValueError(f"march cache of {t.numel()} floats is not [rays][{MARCH_CACHE_ROWS}][{cap}]")
    v = t.detach().view(-1, MARCH_CACHE_ROWS, int(cap))
    fill(v, fpat, ival)
    iv = v.view(torch.int32)
    for r in MARCH_CACHE_INT_ROWS:
        iv[:, r].fill_(int(ival))


def fill_as_bf16(t: torch.Tensor, fpat: float, ival: int) -> None:
    """A byte buffer that holds bf16 operands (``X16``)."""
    fill(t.detach().view(torch.bfloat16), fpat, ival)


# storage address -> cap of a march cache, noted by the allocation hook (the cache is reallocated only by _march_plan)
_MARCH_CACHE_CAP: Dict[int, int] = {}


def _storage_ptr(t: torch.Tensor) -> int:
    return t.untyped_storage().data_ptr()


# ---- the allocation hook -------------------------------------------------------------------------------------------------
# Allocation sites whose buffer needs more than "floats fpat, integers ival": recognised by the caller's module and
# function (sys._getframe), each with the use that makes it index-bearing.
INDEX_SITES = (
    dict(module="esr_nerf_amd.fine_engine", function="_march_plan", what="ws.cache (local `need` floats)",
         use="csrc/march.hip:222 (info >> 8: record offset), :226 / :241 (step), :355, :406",
         treatment="fill_march_cache: rows step / info get ival as int32 bits"),
    dict(module="esr_nerf_amd.fine_engine", function="ensure", what='_Workspace.buf["X16"] (local k == "X16")',
         use="csrc/mlp_bf16.hip: bf16 operands in a uint8 buffer (data, no index)",
         treatment="fill_as_bf16"),
)


class poisoned_allocations:
    """``with poisoned_allocations(fpat, ival) as pa:`` -- for its duration ``torch.empty``, ``torch.empty_like``,
    ``torch.empty_strided`` and ``Tensor.new_empty`` fill what they return (``fill``) when ``device_filter(tensor)`` holds
    (default: device tensors; CPU and pinned tensors are left alone).  On exit -- also after an exception -- the originals are
    restored exactly.  ``pa.allocations`` / ``pa.bytes``: what was filled."""

    _FUNCS = ("empty", "empty_like", "empty_strided")

    def __init__(self, fpat: float, ival: int, device_filter: Callable[[torch.Tensor], bool] = is_device_tensor):
        self.fpat, self.ival, self.device_filter = fpat, ival, device_filter
        self.allocations = 0
        self.bytes = 0
        self._saved = None

    def _filled(self, t, frame):
        if not torch.is_tensor(t) or not self.device_filter(t) or t.numel() == 0:
            return t
        code, mod = frame.f_code.co_name, frame.f_globals.get("__name__")
        loc = frame.f_locals
        if mod == "esr_nerf_amd.fine_engine" and code == "_march_plan" and loc.get("need") is not None \
                and t.numel() == loc["need"] and loc.get("n"):
            cap = int(loc["need"]) // (MARCH_CACHE_ROWS * int(loc["n"]))
            _MARCH_CACHE_CAP[_storage_ptr(t)] = cap
            fill_march_cache(t, cap, self.fpat, self.ival)
        elif mod == "esr_nerf_amd.fine_engine" and code == "ensure" and loc.get("k") == "X16" and t.dtype == torch.uint8:
            fill_as_bf16(t, self.fpat, self.ival)
        else:
            fill(t, self.fpat, self.ival)
        self.allocations += 1
        self.bytes += t.numel() * t.element_size()
        return t

    def __enter__(self):
        if self._saved is not None:
            raise RuntimeError("poisoned_allocations is not re-entrant")
        saved = {name: getattr(torch, name) for name in self._FUNCS}
        own_new_empty = "new_empty" in torch.Tensor.__dict__
        new_empty = torch.Tensor.new_empty
        self._saved = (saved, own_new_empty, torch.Tensor.__dict__.get("new_empty"))
        me = self

        def wrap(orig):
            def poisoned(*args, **kw):
                return me._filled(orig(*args, **kw), sys._getframe(1))
            poisoned.__name__ = getattr(orig, "__name__", "empty")
            poisoned.__wrapped__ = orig
            return poisoned

        for name, orig in saved.items():
            setattr(torch, name, wrap(orig))

        def poisoned_new_empty(self_t, *args, **kw):
            return me._filled(new_empty(self_t, *args, **kw), sys._getframe(1))
        torch.Tensor.new_empty = poisoned_new_empty
        return self

    def __exit__(self, et, ev, tb):
        saved, own_new_empty, orig_new_empty = self._saved
        self._saved = None
        for name, orig in saved.items():
            setattr(torch, name, orig)
        if own_new_empty:
            torch.Tensor.new_empty = orig_new_empty
        else:
            del torch.Tensor.new_empty          # back to the inherited method
        return False


# ---- the SCRATCH / STATE table ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Entry:
    """One row of the table: ``cls`` for every tensor under (owner class, attribute), or -- ``names`` -- per name of the
    innermost dict key it sits under: a list of (regex, SCRATCH | STATE, note); a name that matches none is unclassified.
    ``note``: who writes it before whom (SCRATCH) / what it carries (STATE).  ``how``: a special fill (index safety)."""
    cls: Optional[str]
    note: str = ""
    names: tuple = ()
    how: Optional[str] = None


# The fine engine's tile-major workspace, by buffer name (fine_engine.FINE_ROWS + FINE_OTHER; checked against the source by
# tests/test_poison_host.py): who writes the live part before whom.  All SCRATCH: nothing in it outlives a step.
FINE_BUFFERS = {
    "X": "feat_fwd writes rows 0..103 of every tile [0, tiles_all), padding lanes zero; read by mlp_fwd(rad), wgrad, feat_bwd",
    "gnorm": "feat_fwd -> feat_bwd (normalisation of the gradient features)",
    "H0": "mlp_fwd(rad) -> mlp_wgrad (sums all 32 lanes of a tile: padding lanes must be harmless)",
    "H1": "as H0", "H2": "as H0",
    "z_off": "mlp_fwd(rad) rows 0..3 -> tone_in_fwd, tone dgrad", "z_emo": "as z_off",
    "lin": "tone_in_fwd -> composite_fwd, composite_bwd",
    "Xt": "tone_in_fwd rows 0..32 -> mlp_fwd(tone), tone_wgrad (recomputes Ht)",
    "Ht": "mlp_fwd(tone) saves masks only on the training path; written in full by evaluate",
    "zt": "mlp_fwd(tone) -> composite_fwd", "rgb": "composite_fwd -> composite_bwd",
    "dzt": "composite_bwd -> tone dgrad, tone_wgrad", "dZt": "never written on the training path (recomputed)",
    "dXt": "lazy: tone dgrad -> tone_in_bwd on the two-launch tone path only",
    "dz": "tone dgrad / tone_in_bwd -> mlp_dgrad(rad), mlp_wgrad",
    "dZ0": "mlp_dgrad(rad) -> mlp_wgrad (sums all 32 lanes)", "dZ1": "as dZ0", "dZ2": "as dZ0",
    "dX": "mlp_dgrad(rad) rows 0..43 (+ colour rows) -> feat_bwd; rows above are never read",
    "dweight": "composite_bwd -> march_bwd", "rec_w": "march_fill -> composite, tone_in_bwd",
    "rec_sdf": "march_fill -> feat_fwd", "dsdf": "march_bwd (cached, fold) -> feat_bwd",
    "M0": "ReLU sign words: mlp_fwd(rad) -> mlp_dgrad(rad)", "M1": "as M0", "M2": "as M0",
    "Mt": "mlp_fwd(tone) -> tone dgrad",
    "rec_ray": "filled with -1 (padding lanes) before the plan wait, then march_fill -> every per-sample kernel [index]",
    "rec_step": "march_fill -> feat_fwd / eval_aux; padding lanes stale, guarded by rec_ray < 0 [index]",
    "X16": "bf16 engine: feat_fwd_x16 -> mlp_fwd(rad), wgrad [bf16 in bytes]",
}

# the coarse engine's workspace (voxurfc.CoarseEngine.ROWS / OTHER) shares X, gnorm, rgb, dweight and the record arrays with the
# fine one; its two nets' buffers carry the net's name
COARSE_BUFFERS = (
    (r"(off|emo)\.(H[01]|M[01]|dZ[01])", SCRATCH, "mlp_fwd saves -> mlp_dgrad / mlp_wgrad (sums all 32 lanes of a tile)"),
    (r"(off|emo)\.(z|dz|dX)", SCRATCH, "mlp_fwd -> shade_fwd / shade_bwd -> mlp_dgrad -> feat_bwd"),
)

# lts_engine.Pass.bufs: name patterns of the ``Pass.buf(...)`` call sites (checked against the source on the CPU)
_NETS = r"(off|emo|tone|brdf|emit)"
PASS_BUFFERS = (
    (r"rec_ray|rec_step", SCRATCH, "march_fill -> per-sample kernels; rec_ray pre-filled with -1 [index]"),
    (r"rec_w|rec_sdf", SCRATCH, "march_fill -> composite / features"),
    (r"(X|gnorm)(\.emit)?", SCRATCH, "feat_fwd -> nets, feat_bwd"),
    (r"lin|Xt|rgb", SCRATCH, "tone_in_fwd / composite_fwd of the pass"),
    (r"dweight|dsdf", SCRATCH, "composite_bwd / march_bwd -> feat_bwd"),
    (_NETS + r"\.(H|M|dZ)\d", SCRATCH, "_net_fwd saves -> _net_bwd (wgrad sums all 32 lanes of a tile)"),
    (_NETS + r"\.(z|dz|dX|da)", SCRATCH, "net outputs / gradients of the pass"),
    (_NETS + r"\.(a|ga)", SCRATCH, "activation outputs (_act / _act_batch: esr_act_* writes every tile [0, tiles)) and their gradients"),
    (r"pbr\.t|pts\.t", SCRATCH, "from_rowmajor: zeroed and written in full before its reader"),
)

_MARCH_FIELDS = (
    (r"rays_o|rays_d|viewdirs|mask_density|sdf", STATE, "the caller's inputs and the model's grids"),
    (r"cnt3|off3|stats", SCRATCH, "march_count writes every ray (overflowing rays too) -> plan, fill, backward [index]"),
    (r"last", SCRATCH, "march_count writes every ray -> loss, march_bwd"),
    (r"cache", SCRATCH, "march_count writes [0, n1) of every row of every ray -> fill, backward read [0, n1) [index rows]"),
)

TABLE: Dict[tuple, Entry] = {
    # -- fine_engine ---------------------------------------------------------------------------------------------------------
    ("_Workspace", "buf"): Entry(None, names=tuple((re.escape(k), SCRATCH, v) for k, v in FINE_BUFFERS.items()) + COARSE_BUFFERS),
    ("_Workspace", "ray_bufs"): Entry(SCRATCH, "cnt3 / off3 / stats per ray count: march_count writes every ray before plan / fill [index]"),
    ("_Workspace", "cache"): Entry(SCRATCH, "march cache: march_count -> march_fill, march_bwd of the same step [index rows]", how="march_cache"),
    ("March", "*"): Entry(None, names=_MARCH_FIELDS),
    ("FineEngine", "plan_dev"): Entry(STATE, "the persistent plan header (cleared by plan_begin, read back by the host)"),
    ("FineEngine", "packed"): Entry(STATE, "packed weights: rewritten by every pack, read by every MLP launch"),
    ("FineEngine", "packed16"): Entry(STATE, "bf16 twins of the packed weights"),
    ("FineEngine", "packed_split"): Entry(STATE, "split-fp16 planes of the packed weights"),
    ("FineEngine", "_raw"): Entry(STATE, "the nets' parameters in reference layout (aliases)"),
    ("FineEngine", "range_flag"): Entry(STATE, "the split kernels' sticky range flag"),
    ("FineEngine", "wgrad_scratch"): Entry(SCRATCH, "partial sums of mlp_wgrad: written by its first phase, read by its second, same call"),
    ("FineEngine", "tone_scratch"): Entry(SCRATCH, "partial sums of tone_wgrad: as wgrad_scratch"),
    ("FineEngine", "_loss_acc"): Entry(SCRATCH, "a carve of the step's one zero fill (fresh torch.zeros per forward)"),
    ("FineEngine", "_amax"): Entry(SCRATCH, "as _loss_acc"),
    ("FineEngine", "_amax_t"): Entry(SCRATCH, "as _loss_acc"),
    ("FineEngine", "loss_pair"): Entry(SCRATCH, "as _loss_acc (the returned loss is a view of it: read it before re-poisoning)"),
    # -- lts_engine ----------------------------------------------------------------------------------------------------------
    ("Pass", "bufs"): Entry(None, names=PASS_BUFFERS),
    ("Pass", "cache"): Entry(SCRATCH, "as _Workspace.cache", how="march_cache"),
    ("Pass", "keep"): Entry(STATE, "keep-alive references (the caller's inputs among them); never read through this list"),
    ("LtsEngine", "inv_order"): Entry(SCRATCH, "lts_ref_order writes every slot -> act_batch of the same step [index]"),
    ("LtsEngine", "_za"): Entry(SCRATCH, "the zero arena: a fresh torch.zeros per step"),
    ("LtsEngine", "last_draws"): Entry(STATE, "the random draws of the last forward (replayed by the range fallback)"),
    ("LtsEngine", "last_point_idx"): Entry(STATE, "the surface points of the last forward"),
    ("LtsEngine", "_eval_draws"): Entry(STATE, "the chunks' scattering draws of the last evaluation"),
    ("LtsEngine", "last_wgrad_jobs"): Entry(STATE, "a record of the last backward's weight-gradient jobs (names and aliases)"),
    # -- trainer -------------------------------------------------------------------------------------------------------------
    ("_Step", "_flat"): Entry(SCRATCH, "the flat gradient buffer: zeroed by _alloc_grads in the prelude (zero_() or, with zero_fill_by, "
                              "_zero_unmarked) before any backward kernel adds into it.  Ranges the live-brick optimizer left "
                              "all-zero and marked (Adam._zeroed) are STATE until the next step consumes the mark", how="flat"),
    ("_Step", "_views"): Entry(SCRATCH, "views of _flat", how="alias"),
    ("_Step", "_ovf_host"): Entry(STATE, "pinned host word"),
    # -- optimizer -----------------------------------------------------------------------------------------------------------
    ("Optimizer", "state"): Entry(STATE, "Adam moments"),
    ("Optimizer", "param_groups"): Entry(STATE, "the parameters"),
    ("Adam", "per_lr"): Entry(STATE, "per-voxel learning rate"),
    ("Adam", "_per_lr_for"): Entry(STATE, "per-voxel learning rate in storage order"),
    ("Adam", "_stats"): Entry(STATE, "the live kernel's counters (zeroed once per step(), read by live_stats())"),
    ("Adam", "name2pg"): Entry(STATE, "the parameters, by group name"),
    ("_Live", "flags"): Entry(STATE, "live-brick flags"),
    ("_Live", "moments"): Entry(STATE, "Adam moments (aliases)"),
    # -- models --------------------------------------------------------------------------------------------------------------
    ("Module", "_parameters"): Entry(STATE, "parameters"),
    ("Module", "_buffers"): Entry(STATE, "buffers"),
    ("Module", "grad"): Entry(SCRATCH, "param.grad: with the trainer steps a view of _Step._flat (filled through it, marks respected); a "
                              "gradient of autograd's own is left alone (an alias is only ever filled through its owner)", how="alias"),
    ("VoxurfF", "_tv_cache"): Entry(None, names=((r"mask", STATE, "the non-empty mask as bytes"),
                                                 (r"work", SCRATCH, "smooth_grad_tv_fwd writes the error field -> smooth_grad_tv_bwd, same step"))),
}
# model constants: plain tensor attributes of the renderers and their sub-modules (set once by the constructor or the
# scale-up event; every one carries meaning)
for _cls, _attrs in {
    "VoxurfF": ("xyz_min", "xyz_max", "mask_xyz_min", "mask_xyz_max", "mask_density", "grad_feat", "voxel_size", "world_size",
                "nonempty_mask", "gradient"),
    "VoxurfC": ("xyz_min", "xyz_max", "mask_xyz_min", "mask_xyz_max", "mask_density", "voxel_size", "world_size",
                "nonempty_mask", "gradient"),
    "DVGO": ("xyz_min", "xyz_max", "voxel_size", "world_size"),
    "DenseGrid": ("xyz_min", "xyz_max", "world_size"),
    "MaskCache": ("xyz_min", "xyz_max", "density"),
}.items():
    for _a in _attrs:
        TABLE[(_cls, _a)] = Entry(STATE, "model constant")


@dataclass
class Hit:
    path: str
    owner: str          # class name of the object that holds the attribute
    attr: str
    name: Optional[str]  # innermost dict key (buffer name) under the attribute, if any
    tensor: torch.Tensor
    cls: Optional[str] = None
    entry: Optional[Entry] = None
    key: Optional[tuple] = None
    holder: object = None


class Unclassified(AssertionError):
    pass


def classify(owner_obj, attr: str, name, table=None):
    """-> (class, entry, key) of a tensor under ``owner_obj.attr`` (``name``: innermost dict key)."""
    table = TABLE if table is None else table
    for k in type(owner_obj).__mro__:
        for a in (attr, "*"):
            e = table.get((k.__name__, a))
            if e is None:
                continue
            if not e.names:
                return e.cls, e, (k.__name__, a)
            probe = str(attr if a == "*" else name)
            for pat, cls, _ in e.names:
                if re.fullmatch(pat, probe):
                    return cls, e, (k.__name__, a)
            return None, e, (k.__name__, a)
    return None, None, None


_C_TYPES = (ctypes.Structure, ctypes.Union, ctypes.Array, ctypes._SimpleCData, ctypes._Pointer)
DESCEND_MODULES = ("esr_nerf_amd",)


def survey(root, table=None, device_filter=is_device_tensor, descend_modules=DESCEND_MODULES) -> List[Hit]:
    """Every device tensor reachable from ``root``: through attributes (objects of the product's modules, nn.Modules and
    optimizers), dicts, lists, tuples and sets; from a model through ``model.engine`` (its ``_engine`` attribute) and the
    engine's passes.  Each with its class by the table (``cls`` None: unclassified)."""
    hits: List[Hit] = []
    seen = set()

    def descendable(o):
        mod = type(o).__module__ or ""
        return any(mod == m or mod.startswith(m + ".") for m in descend_modules)

    def visit(o, owner, attr, name, path):
        if torch.is_tensor(o):
            if device_filter(o):
                cls, entry, key = classify(owner, attr, name, table)
                hits.append(Hit(path, type(owner).__name__, attr, name, o, cls, entry, key, owner))
            return
        if o is None or isinstance(o, (str, bytes, int, float, bool, complex, type)) or isinstance(o, _C_TYPES):
            return
        if id(o) in seen:
            return
        seen.add(id(o))
        if isinstance(o, dict):
            for k, v in list(o.items()):
                visit(v, owner, attr, k if isinstance(k, str) else name, f"{path}[{k!r}]" if not torch.is_tensor(k) else f"{path}[<tensor>]")
            return
        if isinstance(o, (list, tuple, set, frozenset)):
            for i, v in enumerate(list(o)):
                visit(v, owner, attr, name, f"{path}[{i}]")
            return
        if isinstance(o, torch.nn.Module):
            for k, p in o._parameters.items():
                if p is not None:
                    visit(p.data, o, "_parameters", k, f"{path}.{k}")
                    if p.grad is not None:
                        visit(p.grad, o, "grad", k, f"{path}.{k}.grad")
            for k, b in o._buffers.items():
                if b is not None:
                    visit(b, o, "_buffers", k, f"{path}.{k}")
            for k, v in list(vars(o).items()):
                if k not in ("_parameters", "_buffers"):
                    visit(v, o, k, None, f"{path}.{k}")
            return
        if isinstance(o, torch.optim.Optimizer):
            for p, st in o.state.items():
                visit(st, o, "state", None, f"{path}.state[...]")
            for k, v in list(vars(o).items()):
                if k != "state":
                    visit(v, o, k, None, f"{path}.{k}")
            return
        if descendable(o):
            d = dict(vars(o)) if hasattr(o, "__dict__") else {}
            for k in getattr(type(o), "__slots__", ()):
                if hasattr(o, k):
                    d[k] = getattr(o, k)
            for k, v in d.items():
                visit(v, o, k, None, f"{path}.{k}")

    roots = root if isinstance(root, (list, tuple)) else [root]
    for i, r in enumerate(roots):
        if isinstance(r, (torch.nn.Module, torch.optim.Optimizer)) or descendable(r):
            visit(r, None, None, None, f"<{type(r).__name__}>")
        else:
            raise TypeError(f"repoison / survey start at an engine, step, model or optimizer object, not {type(r).__name__}")
    return hits


@dataclass
class Report:
    filled: int = 0                 # storages filled
    bytes: int = 0
    storages: int = 0               # distinct storages reached
    state: int = 0                  # storages left alone
    names: tuple = ()               # (path, bytes) of what was filled


def _marked_ranges(step, flat):
    """Element ranges of ``flat`` that ``step.zero_fill_by`` (optimizer.Adam with zero_grads) holds a mark for: left all-zero
    by its live kernel, and trusted by ``_Step._zero_unmarked`` -- STATE until the next step consumes the mark."""
    opt = getattr(step, "zero_fill_by", None)
    out = []
    if opt is None:
        return out
    base, size = flat.data_ptr(), flat.element_size()
    for dev, ptr, numel in getattr(opt, "_zeroed", ()):
        if dev == flat.device and base <= ptr and ptr + numel * size <= base + flat.numel() * size:
            out.append(((ptr - base) // size, (ptr - base) // size + numel))
    return sorted(out)


def repoison(root, fpat: float, ival: int, table=None, device_filter=is_device_tensor,
             descend_modules=DESCEND_MODULES, cache_cap: Optional[Callable[[torch.Tensor], int]] = None) -> Report:
    """Fill every device tensor reachable from ``root`` that the table classifies SCRATCH; leave STATE bit-identical; raise
    ``Unclassified`` for a tensor in neither class.  Each storage is visited once: when several tensors share one, STATE
    wins (nothing of it is touched), otherwise the owner's view is filled -- the one with a special fill, else the largest;
    a storage reached through aliases only (``how="alias"``: ``_Step._views``, ``param.grad``) is left alone."""
    hits = survey(root, table, device_filter, descend_modules)
    bad = [h for h in hits if h.cls is None]
    if bad:
        raise Unclassified("device tensors in neither class (add them to tests/poison.py TABLE, with who writes them before whom): "
                           + "; ".join(f"{h.path} (owner {h.owner}, attribute {h.attr}, name {h.name}, {tuple(h.tensor.shape)} {h.tensor.dtype})"
                                       for h in bad[:12]))
    groups: Dict[int, List[Hit]] = {}
    for h in hits:
        if h.tensor.numel():
            groups.setdefault(_storage_ptr(h.tensor), []).append(h)
    rep, names = Report(storages=len(groups)), []
    for ptr, hs in groups.items():
        if any(h.cls == STATE for h in hs) or all(h.entry.how == "alias" for h in hs):
            rep.state += 1              # (aliases alone: their owner is out of reach, nothing says the storage is scratch)
            continue
        special = [h for h in hs if h.entry.how not in (None, "alias")]
        h = special[0] if special else max(hs, key=lambda x: x.tensor.numel())
        t, how = h.tensor, h.entry.how
        if how == "march_cache" or (h.owner == "March" and h.attr == "cache"):
            cap = cache_cap(t) if cache_cap is not None else _MARCH_CACHE_CAP.get(ptr)
            if cap is None:
                raise Unclassified(f"{h.path}: a march cache whose row length is unknown (allocated outside poisoned_allocations?)")
            fill_march_cache(t, cap, fpat, ival)
        elif how == "flat":
            lo = 0
            for a, b in _marked_ranges(h.holder, t) + [(t.numel(), t.numel())]:
                if a > lo:
                    fill(t[lo:a], fpat, ival)
                lo = max(lo, b)
        elif h.name == "X16" and t.dtype == torch.uint8:
            fill_as_bf16(t, fpat, ival)
        else:
            fill(t, fpat, ival)
        rep.filled += 1
        rep.bytes += t.numel() * t.element_size()
        names.append((h.path, t.numel() * t.element_size()))
    rep.names = tuple(names)
    return rep


# ---- comparing two legs ----------------------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


def _rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    """conftest.rel_err: max |a - b| / max |b|."""
    a, b = a.detach().double(), b.detach().double()           # (on the tensors' device: whole grids are compared)
    if b.numel() == 0:
        return 0.0 if a.numel() == 0 else float("inf")
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _flatten(d, prefix=""):
    out = {}
    if isinstance(d, dict):
        for k, v in d.items():
            out.update(_flatten(v, f"{prefix}{k}" if not prefix else f"{prefix}/{k}"))
    elif isinstance(d, (list, tuple)):
        for i, v in enumerate(d):
            out.update(_flatten(v, f"{prefix}[{i}]"))
    else:
        out[prefix] = d
    return out


def compare(a: dict, b: dict, deterministic=(), bar: float = BAR_FINE) -> Dict[str, float]:
    """``a``: the results of leg A (the twin), ``b``: those of a poisoned leg -- dictionaries (nested dicts / lists allowed)
    of outputs, loss, gradients and counters.  Raises ``Mismatch`` unless
      * both hold the same keys,
      * every float of ``b`` is finite wherever it is finite in ``a``,
      * counters and integer / bool outputs are equal,
      * float outputs whose key (or its first path component) is listed ``deterministic`` are ``torch.equal`` with equal
        sign bits,
      * every other float output is within ``rel_err < bar`` of ``a`` (the bar of two runs of the same step).
    -> {key: rel_err} of the non-deterministic float outputs."""
    fa, fb = _flatten(a), _flatten(b)
    if set(fa) != set(fb):
        raise Mismatch(f"different result keys: {sorted(set(fa) ^ set(fb))}")
    det = set(deterministic)
    errs, bad = {}, []
    for k in fa:
        x, y = fa[k], fb[k]
        if isinstance(x, float) and not torch.is_tensor(y):
            x, y = torch.tensor(x, dtype=torch.float64), torch.tensor(float(y), dtype=torch.float64)
        if not torch.is_tensor(x):
            if torch.is_tensor(y) or x != y:
                bad.append(f"{k}: {x!r} != {y!r}")
            continue
        if not torch.is_tensor(y) or x.shape != y.shape or x.dtype != y.dtype:
            bad.append(f"{k}: shape / type differ")
            continue
        if not x.is_floating_point():
            if not torch.equal(x, y):
                bad.append(f"{k}: integer output differs in {int((x != y).sum())} places")
            continue
        fin = torch.isfinite(x)
        if not bool(torch.isfinite(y)[fin].all()):
            bad.append(f"{k}: {int((~torch.isfinite(y) & fin).sum())} non-finite values where the twin is finite")
            continue
        if k in det or k.split("/")[0] in det:
            same = torch.equal(x[fin], y[fin]) and torch.equal(torch.signbit(x), torch.signbit(y)) \
                and torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.isfinite(x), torch.isfinite(y))
            if not same:
                bad.append(f"{k}: deterministic output differs (rel_err {_rel_err(y[fin], x[fin]):.3e})")
            continue
        e = _rel_err(y[fin], x[fin])
        errs[k] = e
        if not e < bar:
            bad.append(f"{k}: rel_err {e:.3e} >= {bar:g}")
    if bad:
        raise Mismatch("; ".join(bad[:10]) + (f" (+{len(bad) - 10} more)" if len(bad) > 10 else ""))
    return errs
