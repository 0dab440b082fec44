"""PDRA's ray re-split: which uncertain rays stay uncertain -- ``update_ray_groups`` of the reference's PDRA trainer
(app/fine/pdra.py:882-932) with ``RayGroupManager.filter`` (utils2/utils.py:234-267) -- over the kernels of
esr_nerf_amd/csrc/regroup.hip.

``decide``             emission [n, 3] -> one flag per ray (``max_c emission > k_val``) and the statistics the reference
                       prints, in one launch; chunk after chunk into one flag vector and one statistics record
``partition``          rows, flags -> ``(rows[flags], rows[~flags])``, both in input order (count, scan, scatter)
``apply_flags``        what ``sampler.filter(flags)`` does, for a ``RayGroupManager`` or a ``CameraRayGroupManager``
``update_ray_groups``  the trainer's method: ``eval_emit`` over the uncertain group in chunks, ``decide`` per chunk,
                       ``apply_flags`` once, the reference's printed lines -> ``RegroupReport``

A PDRA trainer calls ``update_ray_groups(self.renderer, self.sampler, self.k_val)`` where the reference calls
``self.update_ray_groups(self.k_val)`` (pdra.py:219 and :372).

Host read-backs.  ``update_ray_groups`` reads back once per call.  For a sampler whose index vectors live on the device
these are 64 bytes (the statistics and the two totals the allocation of the new vectors needs); a ``data_preload: cpu``
sampler keeps its index vectors on the host, so the flags travel in the same copy, in front of the statistics, and the
existing ``filter`` lines run on them.  (``eval_emit`` itself reads its march plan back per chunk; that is the engine's.)

Fine-tune mode.  The mode is put back as ``relight.EditRaySelector`` does, with ``renderer.train(True, finetune=True)``, and
``ESRNeRF.train`` then freezes a NEW copy of the current ``emo_color`` as ``emit_color`` (esrnerf.py:218-239): a re-split in
the middle of a fine-tune replaces the frozen emission grid by the trained one.  The PDRA trainer re-splits in plain
training mode only (pdra.py:219, :372).

Data parallelism is not implemented here, but the seam is fixed: the groups change ONLY through ``apply_flags``, which is a
deterministic function of the flags.  With ``world > 1`` every rank holds the full index vectors, so all ranks MUST call
``apply_flags`` with the SAME flags -- one rank's flags broadcast, or per-rank shares all-gathered -- never with flags each
rank decided for itself (a ray on the boundary may be decided differently by two ranks, and the index vectors would diverge).
``update_ray_groups`` on a sampler with ``world > 1`` therefore raises ``NotImplementedError``.

There is no CPU kernel: ``decide`` and ``partition`` raise on CPU tensors.  ``update_ray_groups`` with a renderer on the CPU
(a stub in the tests) takes the reference's torch statements for the decision.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from . import _lib

# rays per ``eval_emit`` pass when the caller names none: the smallest measured size whose time is within 5 % of the best
# (tools/regroup_time.py, profiles/regroup_time.json, DESIGN.md: 2.3 x the retained loop at chunk 4096; the engine keeps
# 9.3 GB of buffers afterwards, 2.7 GB at 16384).  The reference's eval.uncert_batch_size = 4096 stays a valid argument.
DEFAULT_BATCH_SIZE = 65536

STAT_KEYS = ("n_set", "n_clear", "n_nan", "min_all", "max_all", "min_set", "max_set", "min_clear", "max_clear")
_STATS_WORDS = C.sizeof(_lib.EsrRegroupStats) // 8             # the record, then totals (set, clear): int64 [6 + 2]
RAY_KEYS = ("rays_o", "rays_d", "viewdirs")


@dataclass
class RegroupReport:
    k_val: float
    uncertain_before: int
    certain_before: int
    uncertain_after: int
    certain_after: int
    stats: Dict[str, float]
    flags: torch.Tensor                          # [uncertain_before] bool, aligned with the uncertain group's order before
    emission: Optional[torch.Tensor] = None      # [uncertain_before, 3], only with return_emission


def _need_device(what: str, *tensors):
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"{what} runs on libesr_hip.so and needs device tensors (there is no CPU kernel)")


def _u8(flags: torch.Tensor) -> torch.Tensor:
    if flags.dtype not in (torch.bool, torch.uint8) or flags.dim() != 1 or not flags.is_contiguous():
        raise ValueError(f"flags are a contiguous bool / uint8 vector, got {flags.dtype} {tuple(flags.shape)}")
    return flags.view(torch.uint8)


def new_stats(device) -> torch.Tensor:
    """An int64 [8] device buffer: ``esr_regroup_stats_t`` (48 bytes) followed by ``totals`` (set, clear)"""
    return torch.empty(_STATS_WORDS + 2, dtype=torch.int64, device=device)


def read_stats(stats: torch.Tensor) -> Dict[str, float]:
    """The statistics record as a host dict (ONE read-back of the whole buffer, totals included as ``totals``)"""
    return _parse_stats(stats.cpu().numpy())


def _parse_stats(host) -> Dict[str, float]:
    rec = _lib.EsrRegroupStats.from_buffer_copy(host[:_STATS_WORDS].tobytes())
    out = {k: getattr(rec, k) for k in STAT_KEYS}
    out["totals"] = (int(host[_STATS_WORDS]), int(host[_STATS_WORDS + 1]))
    return out


@torch.no_grad()
def decide(emission: torch.Tensor, k_val: float, flags: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None):
    """emission [n, 3] float32 device tensor -> ``(flags, stats)``: ``flags`` [n] bool (``max_c emission > k_val`` as a
    binary32 comparison; a ray with a NaN channel is not set), written into the given vector (bool or uint8, e.g. a slice
    of a longer one) or a new one; ``stats`` the device buffer of ``new_stats`` -- a given one is MERGED into (chunk after
    chunk), without one a new record is started.  One launch on the current stream, not waited for; ``read_stats`` reads."""
    _need_device("decide", emission)
    if emission.dim() != 2 or emission.shape[1] != 3 or emission.dtype != torch.float32:
        raise ValueError(f"decide: emission is [n, 3] float32, got {emission.dtype} {tuple(emission.shape)}")
    dev = emission.device
    e = emission.contiguous()
    n = int(e.shape[0])
    with torch.cuda.device(dev):
        if flags is None:
            flags = torch.empty(n, dtype=torch.bool, device=dev)
        if len(flags) != n or flags.device != dev:
            raise ValueError(f"decide: {n} rays on {dev}, flags {tuple(flags.shape)} on {flags.device}")
        accumulate = stats is not None
        if stats is None:
            stats = new_stats(dev)
            if n == 0:                                   # (the entry point touches nothing for n == 0)
                stats.copy_(_identity().to(dev))
        _lib.check(_lib.lib().esr_emit_decide(_lib.ptr(e), n, float(k_val), _lib.ptr(_u8(flags)), _lib.ptr(stats),
                                              int(accumulate), _lib.stream_ptr(dev)), "esr_emit_decide")
    return (flags if flags.dtype == torch.bool else flags.view(torch.bool)), stats


def _identity() -> torch.Tensor:
    inf = float("inf")
    rec = _lib.EsrRegroupStats(0, 0, 0, inf, -inf, inf, -inf, inf, -inf)
    return torch.frombuffer(bytearray(bytes(rec)) + bytearray(16), dtype=torch.int64).clone()


def _scan(flags_u8: torch.Tensor, totals: torch.Tensor) -> torch.Tensor:
    dev = flags_u8.device
    n = int(flags_u8.numel())
    off = torch.empty((n + _lib.PARTITION_BLOCK - 1) // _lib.PARTITION_BLOCK, dtype=torch.int64, device=dev)
    if n == 0:
        totals.zero_()
    _lib.check(_lib.lib().esr_flag_scan(_lib.ptr(flags_u8), n, _lib.ptr(off), _lib.ptr(totals), _lib.stream_ptr(dev)),
               "esr_flag_scan")
    return off


def _scatter(rows, flags_u8, off, set_out, clear_out):
    dev = rows.device
    _lib.check(_lib.lib().esr_index_partition(_lib.ptr(rows), _lib.ptr(flags_u8), _lib.ptr(off), int(rows.numel()),
                                              _lib.ptr(set_out), _lib.ptr(clear_out), _lib.stream_ptr(dev)),
               "esr_index_partition")


def _check_rows(what, rows, flags):
    if rows.dtype != torch.int64 or rows.dim() != 1 or len(flags) != len(rows) or flags.device != rows.device:
        raise ValueError(f"{what}: rows are an int64 vector with one flag each on one device, got {rows.dtype} "
                         f"{tuple(rows.shape)} on {rows.device} and flags {tuple(flags.shape)} on {flags.device}")


@torch.no_grad()
def partition(rows: torch.Tensor, flags: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(rows[flags], rows[~flags])`` for an int64 device vector and its bool / uint8 flags, both in input order.  Reads the
    two totals back (the results are allocated at their exact sizes)."""
    _need_device("partition", rows, flags)
    _check_rows("partition", rows, flags)
    dev = rows.device
    f, r = _u8(flags), rows.contiguous()
    with torch.cuda.device(dev):
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        off = _scan(f, totals)
        n_set, n_clear = totals.tolist()
        set_rows = torch.empty(n_set, dtype=torch.int64, device=dev)
        clear_rows = torch.empty(n_clear, dtype=torch.int64, device=dev)
        _scatter(r, f, off, set_rows, clear_rows)
    return set_rows, clear_rows


@torch.no_grad()
def apply_flags(sampler, flags: torch.Tensor, stats: Optional[torch.Tensor] = None) -> Optional[Dict[str, float]]:
    """``sampler.filter(flags)``: a set flag keeps its ray uncertain, a clear one moves it to the END of the certain group;
    ``uncert_batch_st`` and ``cert_batch_st`` stay as they are.  ``flags`` is aligned with the uncertain group's current
    order.  Index vectors on the device: scan, one read-back (of ``stats`` when given, whose last two words take the
    totals), exact-size allocation, a device copy of the old certain vector, the partition.  A ``data_preload: cpu`` sampler:
    the existing ``filter`` lines.  With ``world > 1`` all ranks must pass the SAME flags (module docstring).
    Returns ``read_stats(stats)`` when ``stats`` is given."""
    rows, old = sampler.uncert_data_idxs, sampler.cert_data_idxs
    if len(flags) != len(rows):
        raise ValueError(f"apply_flags: {len(flags)} flags for an uncertain group of {len(rows)} rays")
    if not rows.is_cuda:
        host = read_stats(stats) if stats is not None else None
        sampler.filter(flags.view(torch.bool) if flags.dtype == torch.uint8 else flags)
        return host
    _need_device("apply_flags", flags)
    _check_rows("apply_flags", rows, flags)
    dev = rows.device
    f = _u8(flags)
    with torch.cuda.device(dev):
        buf = stats if stats is not None else new_stats(dev)
        off = _scan(f, buf[_STATS_WORDS:])
        host = read_stats(buf)
        n_set, n_clear = host["totals"]
        new_u = torch.empty(n_set, dtype=torch.int64, device=dev)
        new_c = torch.empty(len(old) + n_clear, dtype=torch.int64, device=dev)
        new_c[:len(old)].copy_(old)
        _scatter(rows.contiguous(), f, off, new_u, new_c[len(old):])
    sampler.uncert_data_idxs, sampler.cert_data_idxs = new_u, new_c
    return host if stats is not None else None


def _merge(a: Optional[Dict[str, float]], b: Dict[str, float]) -> Dict[str, float]:
    if a is None:
        return b
    return {k: (a[k] + b[k] if k.startswith("n_") else min(a[k], b[k]) if k.startswith("min") else max(a[k], b[k]))
            for k in STAT_KEYS}


def _decide_torch(emission: torch.Tensor, k_val: float):
    """The reference's statements (pdra.py:911-925) for CPU tensors; minima and maxima over the non-NaN values"""
    inf = float("inf")
    flags = torch.max(emission, dim=-1)[0] > k_val
    nan = torch.isnan(emission)

    def lo_hi(sel):
        v = emission[sel][~nan[sel]]
        return (float(v.min()), float(v.max())) if v.numel() else (inf, -inf)

    every = torch.ones_like(flags)
    (la, ha), (ls, hs), (lc, hc) = lo_hi(every), lo_hi(flags), lo_hi(~flags)
    n_set = int(flags.sum())
    return flags, dict(n_set=n_set, n_clear=len(flags) - n_set, n_nan=int(nan.any(-1).sum()), min_all=la, max_all=ha,
                       min_set=ls, max_set=hs, min_clear=lc, max_clear=hc)


def _chunk_rays(sampler, rows: torch.Tensor, dev: torch.device) -> Dict[str, torch.Tensor]:
    """The three ray arrays of the original rows ``rows`` on the device: made by the camera kernel for a camera set, gathered
    from ``sampler.data`` otherwise (a CPU home: into pinned memory, then a non-blocking upload)."""
    if hasattr(sampler, "cams"):
        from .camera import camera_batch
        made = camera_batch(sampler.cams, sampler.images, sampler.em_modes, rows, sampler.white_bg, check_rows=False)
        return {k: made[k] for k in RAY_KEYS}
    if rows.is_cuda or dev.type != "cuda":
        return {k: sampler.data[k][rows].to(dev, non_blocking=True) for k in RAY_KEYS}
    out = {}
    for k in RAY_KEYS:
        src = sampler.data[k]
        stage = torch.empty((len(rows), *src.shape[1:]), dtype=src.dtype, pin_memory=True)
        torch.index_select(src, 0, rows, out=stage)
        out[k] = stage.to(dev, non_blocking=True)
    return out


def _stats_line(sampler) -> str:
    """utils2/utils.py:305-312 (print_stats)"""
    nu, nc = sampler.uncert_data_num, sampler.cert_data_num
    share = nu / (nu + nc) * 100 if nu + nc else float("nan")
    return f"uncertain: {nu}\t certain: {nc}\t uncertain/all: {share}"


@torch.no_grad()
def update_ray_groups(renderer, sampler, k_val: float, batch_size: Optional[int] = None, verbose: bool = True,
                      return_emission: bool = False) -> RegroupReport:
    """pdra.py:882-932: ``renderer.eval_emit`` on every ray of the sampler's uncertain group in its current order,
    ``batch_size`` rays per pass (None: ``DEFAULT_BATCH_SIZE``); a ray stays uncertain iff ``max_c emission > k_val``, all
    others go to the end of the certain group.  The renderer is in ``eval()`` for the duration and gets its mode (train or
    fine-tune) back afterwards, also when ``eval_emit`` raises.  No [n, 3] emission buffer is kept unless
    ``return_emission``.  ``verbose`` prints the reference's lines."""
    if getattr(sampler, "world", 1) > 1:
        raise NotImplementedError(
            "update_ray_groups: data parallelism is not implemented -- with world > 1 every rank holds the full index "
            "vectors, so all ranks must call apply_flags with the SAME flags (one rank's flags, or all-gathered shares)")
    bs = DEFAULT_BATCH_SIZE if batch_size is None else int(batch_size)
    if bs < 1:
        raise ValueError("update_ray_groups: batch_size must be positive")
    k_val = float(k_val)
    dev = torch.device(sampler.device)
    on_device = dev.type == "cuda"
    all_rows = sampler.uncert_data_idxs
    n = len(all_rows)
    before = (sampler.uncert_data_num, sampler.cert_data_num)
    if verbose:
        print("[PREV]\n" + _stats_line(sampler) + f"\ncurr k_val: {k_val}")
    # one device buffer: the flags, then (8-byte aligned) the statistics record and the totals -- a CPU-home sampler
    # reads all of it back in one copy
    n_pad = (n + 7) // 8 * 8
    store = torch.empty(n_pad + 8 * (_STATS_WORDS + 2), dtype=torch.uint8, device=dev)
    flags = store[:n].view(torch.bool)
    emission = torch.empty(n, 3, dtype=torch.float32, device=dev) if return_emission else None
    stats_dev, stats = None, None
    if on_device:
        stats_dev = store[n_pad:].view(torch.int64)
        stats_dev.copy_(_identity())
    was_training = renderer.training
    finetune = was_training and getattr(renderer, "forward", None) == getattr(renderer, "forward_finetune", None)
    renderer.eval()
    try:
        for a in range(0, n, bs):
            rows = all_rows[a:a + bs]
            e = renderer.eval_emit(**_chunk_rays(sampler, rows, dev))
            if on_device:
                decide(e, k_val, flags[a:a + len(rows)], stats_dev)
            else:
                flags[a:a + len(rows)], part = _decide_torch(e, k_val)
                stats = _merge(stats, part)
            if return_emission:
                emission[a:a + len(rows)].copy_(e)
    finally:
        if was_training:
            renderer.train(True, finetune=True) if finetune else renderer.train(True)
    if on_device and all_rows.is_cuda:
        stats = apply_flags(sampler, flags, stats_dev)
        stats.pop("totals")
    elif on_device:
        host = store.cpu()
        stats = _parse_stats(host[n_pad:].view(torch.int64).numpy())
        stats.pop("totals")
        sampler.filter(host[:n].view(torch.bool))
    else:
        if stats is None:
            stats = _decide_torch(torch.empty(0, 3), k_val)[1]
        apply_flags(sampler, flags)
    if verbose:
        # pdra.py:912-925; the reference prints the three pairs only for a non-empty selection
        if n:
            print("emission(max, min):", stats["max_all"], stats["min_all"])
        if stats["n_set"]:
            print("emission_uncert_masks(max, min):", stats["max_set"], stats["min_set"])
        if stats["n_clear"]:
            print("emission_cert_masks(max, min):", stats["max_clear"], stats["min_clear"])
        print("[NEW MASK UPDATE]\n" + _stats_line(sampler))
    return RegroupReport(k_val, before[0], before[1], sampler.uncert_data_num, sampler.cert_data_num, stats, flags, emission)
