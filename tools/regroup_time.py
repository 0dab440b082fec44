"""Times of PDRA's ray re-split (esr_nerf_amd/regroup.py) on the device.

    python tools/regroup_time.py [--rays 1048576] [--rows 64000000] [--share-rows 67108864] [--repeats 5] [--rounds 3]
                                 [--kernels-only] [--out profiles/regroup_time.json]

The case of tools/relight_time.py: the C2 slab scene with ``--rays`` rays, all uncertain, the index vectors on the device;
``k_val`` is the median of the per-ray maxima, so about half of the rays move.  Device events around whole calls (host time
included: the loops are host-bound at small chunks), one warm-up, ``--repeats`` runs per round and their median, ``--rounds``
rounds interleaving every variant; the spread reported is that of the rounds' medians.
  (a) the retained loop: the reference's statements (app/fine/pdra.py:887-927, the printed reductions evaluated as the prints
      evaluate them) over this package's ``eval_emit`` and ``RayGroupManager.filter`` at chunk 4096
  (b) ``update_ray_groups`` (verbose, so the statistics are read) at chunks 4096, 16384, 65536 and 262144, with the peak
      device memory of a call and what stays allocated after it (the engine keeps the buffers of its largest chunk)
  (c) ``apply_flags`` on byte flags (pack + flag scan + read-back + allocation + copy of the old certain vector + partition)
      against ``RayGroupManager.filter`` (two boolean indexings + cat) on ``--rows`` int64 rows, and the three entry points
      ``esr_flags_pack``, ``esr_flag_scan_bits`` and ``esr_index_partition_bits`` alone
  (d) the device work of a single-process re-split behind ``eval_emit``: ``esr_emit_decide`` + ``esr_flags_pack`` +
      ``esr_flag_scan_bits`` + ``esr_index_partition_bits`` on ``--share-rows`` rows (2^26) at set shares 1 %, 50 % and 99 %
      (emission uniform in [0, 1), ``k_val = (1 - share)^(1/3)``), ``2 * --repeats`` runs per round
``--kernels-only`` runs (c) and (d) alone.  Per-ray times are also scaled to 64 M rays (100 views of 800 x 800).  The default
chunk is the smallest measured size whose time is within 5 % of the best.  One JSON line.
"""
import argparse
import contextlib
import io
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNKS = (4096, 16384, 65536, 262144)
SHARES = (0.01, 0.5, 0.99)
USER_RAYS = 64_000_000


def run_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def retained_loop(renderer, sampler, k_val, bs):
    """pdra.py:887-927 over eval_emit and RayGroupManager.filter: the [n,3] buffer, the indexed result copy, the five
    reductions of the prints (a print needs the value on the host), filter"""
    dev = torch.device(sampler.device)
    rays_o, rays_d, viewdirs = (sampler.uncert(k) for k in ("rays_o", "rays_d", "viewdirs"))
    emission = torch.zeros_like(rays_o)
    renderer.eval()
    for idx in torch.arange(len(emission), device=dev).split(bs):
        emission[idx] = renderer.eval_emit(rays_o=rays_o[idx].to(dev), rays_d=rays_d[idx].to(dev), viewdirs=viewdirs[idx].to(dev))
    mask = torch.max(emission, dim=-1)[0] > k_val
    lines = []
    if emission.numel():
        lines.append(f"emission(max, min): {emission.max()} {emission.min()}")
    if mask.sum():
        lines.append(f"emission_uncert_masks(max, min): {emission[mask].max()} {emission[mask].min()}")
    if mask.bitwise_not().sum():
        lines.append(f"emission_cert_masks(max, min): {emission[mask.bitwise_not()].max()} {emission[mask.bitwise_not()].min()}")
    sampler.filter(mask)
    renderer.train()
    return mask, lines


def summary(per_round, n_rays):
    med = [float(np.median(r)) for r in per_round]
    m = float(np.median(med))
    return dict(ms_round_medians=[round(v, 3) for v in med], ms=round(m, 3), spread=round((max(med) - min(med)) / m, 4),
                ns_per_ray=round(m * 1e6 / n_rays, 4), ms_at_64M_rays=round(m * USER_RAYS / n_rays, 1))


def loop_section(a):
    """(a) and (b)"""
    from esr_nerf_amd import regroup
    from esr_nerf_amd.config import lts_cfg
    from esr_nerf_amd.data import RayGroupManager
    from esr_nerf_amd.esrnerf import ESRNeRF
    from esr_nerf_amd.synthetic import init_slab_model, slab_scene

    dev, n = torch.device("cuda:0"), a.rays
    sc = slab_scene("C2", s_val=60.0, oblique=True, n_rays=n)
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = lts_cfg("cuda:0")
    cfg.system["data_preload"] = "cuda"
    m = init_slab_model(ESRNeRF(cfg, sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max,
                                sc.mask_alpha_init, sc.mask_density, sc.s_val, sc.num_voxels), sc)
    m.s_val = sc.s_val
    m.train()
    keys = ["rays_o", "rays_d", "viewdirs", "em_modes"]
    s = RayGroupManager(cfg, {k: sc.batch[k] for k in keys}, keys, 4096, 4096,
                        uncert_data_idxs=torch.randperm(n, generator=torch.Generator().manual_seed(0)))
    base = s.uncert_data_idxs

    def reset():
        s.uncert_data_idxs, s.cert_data_idxs = base, base[:0]

    quiet = contextlib.redirect_stdout(io.StringIO())
    # k_val: the median per-ray maximum (untimed; this run is also the warm-up of the 4096 chunk)
    reset()
    with quiet:
        rep = regroup.update_ray_groups(m, s, 0.0, batch_size=4096, return_emission=True)
    k_val = float(rep.emission.max(1)[0].median())
    del rep

    variants = {"retained_loop_4096": lambda: retained_loop(m, s, k_val, 4096)}
    for c in CHUNKS:
        variants[f"update_ray_groups_{c}"] = (lambda c=c: regroup.update_ray_groups(m, s, k_val, batch_size=c))
    memory, flags_of = {}, {}
    for name, fn in variants.items():                       # warm-up in ascending chunk order, with the memory figures
        reset()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        with quiet:
            r = fn()
        torch.cuda.synchronize()
        flags_of[name] = (r[0] if isinstance(r, tuple) else r.flags).clone()
        del r
        reset()
        memory[name] = dict(allocated_before_mb=round(before / 2 ** 20, 1),
                            peak_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1),
                            allocated_after_mb=round(torch.cuda.memory_allocated() / 2 ** 20, 1))
    ref_flags = flags_of["retained_loop_4096"]
    differ = {k: int((v != ref_flags).sum()) for k, v in flags_of.items()}
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            ms = []
            for _ in range(a.repeats):
                reset()
                with quiet:
                    ms.append(run_ms(fn))
            times[name].append(ms)
    reset()
    loop = {k: dict(summary(v, n), **memory[k], flags_differing_from_retained_loop=differ[k]) for k, v in times.items()}
    best = min(loop[f"update_ray_groups_{c}"]["ms"] for c in CHUNKS)
    default = next(c for c in CHUNKS if loop[f"update_ray_groups_{c}"]["ms"] <= 1.05 * best)
    base_ms = loop["retained_loop_4096"]["ms"]
    ratios = {str(c): round(base_ms / loop[f"update_ray_groups_{c}"]["ms"], 3) for c in CHUNKS}
    return dict(scene="C2 slab", rays=n, k_val=k_val, loop=loop, speedup_over_retained_loop=ratios, default_batch_size=default)


def partition_section(a):
    """(c) the partition alone on --rows rows"""
    from esr_nerf_amd import _lib, regroup
    dev = torch.device("cuda:0")
    N = a.rows
    g = torch.Generator(device=dev).manual_seed(1)
    rows = torch.randperm(N, device=dev, generator=g)
    flags = torch.rand(N, device=dev, generator=g) < 0.5
    old = torch.arange(N, N + a.old_certain, device=dev)
    ours, theirs = SimpleNamespace(), SimpleNamespace()

    def ours_fn():
        ours.uncert_data_idxs, ours.cert_data_idxs = rows, old
        regroup.apply_flags(ours, flags)

    def torch_fn():                                          # RayGroupManager.filter's lines (data.py)
        theirs.uncert_data_idxs, theirs.cert_data_idxs = rows, old
        theirs.cert_data_idxs = torch.cat([theirs.cert_data_idxs, theirs.uncert_data_idxs[~flags]]).contiguous()
        theirs.uncert_data_idxs = theirs.uncert_data_idxs[flags].contiguous()

    f8 = flags.view(torch.uint8)
    words = torch.empty(regroup.n_words(N), dtype=torch.int64, device=dev)
    off = torch.empty((N + _lib.PARTITION_BLOCK - 1) // _lib.PARTITION_BLOCK, dtype=torch.int64, device=dev)
    tot = torch.empty(2, dtype=torch.int64, device=dev)
    so, co = torch.empty(N, dtype=torch.int64, device=dev), torch.empty(N, dtype=torch.int64, device=dev)
    L, sp = _lib.lib(), _lib.stream_ptr(dev)
    part = {"apply_flags": ours_fn, "torch_filter_lines": torch_fn,
            "esr_flags_pack": lambda: L.esr_flags_pack(_lib.ptr(f8), N, _lib.ptr(words), sp),
            "esr_flag_scan_bits": lambda: L.esr_flag_scan_bits(_lib.ptr(words), N, _lib.ptr(off), _lib.ptr(tot), sp),
            "esr_index_partition_bits": lambda: L.esr_index_partition_bits(_lib.ptr(rows), _lib.ptr(words), _lib.ptr(off), N,
                                                                           _lib.ptr(so), _lib.ptr(co), sp)}
    ptimes = {k: [] for k in part}
    for fn in part.values():
        fn()
    torch.cuda.synchronize()
    equal = bool(torch.equal(ours.uncert_data_idxs, theirs.uncert_data_idxs) and torch.equal(ours.cert_data_idxs, theirs.cert_data_idxs))
    for _ in range(a.rounds):
        for name, fn in part.items():
            ptimes[name].append([run_ms(fn) for _ in range(2 * a.repeats)])
    partition = {k: summary(v, N) for k, v in ptimes.items()}
    moved = N * (8 + 8) + N // 8
    partition["esr_index_partition_bits"]["tb_per_s"] = round(moved / (partition["esr_index_partition_bits"]["ms"] * 1e-3) / 1e12, 3)
    partition["speedup_apply_flags_over_torch"] = round(partition["torch_filter_lines"]["ms"] / partition["apply_flags"]["ms"], 3)
    return dict(partition_rows=N, old_certain_rows=a.old_certain, partition=partition, partition_equals_torch=equal)


def resplit_kernels_at(n, share, repeats, rounds):
    """(d) decide into bytes + pack + scan + partition on n rows at one set share"""
    from esr_nerf_amd import _lib
    dev = torch.device("cuda:0")
    L, sp, p = _lib.lib(), _lib.stream_ptr(dev), _lib.ptr
    g = torch.Generator(device=dev).manual_seed(int(share * 100))
    e = torch.rand(n, 3, device=dev, generator=g)
    k_val = float((1.0 - share) ** (1.0 / 3.0))
    rows = torch.randperm(n, device=dev, generator=g)
    new = lambda m, dt=torch.int64: torch.empty(m, dtype=dt, device=dev)
    flags, words = new(n, torch.uint8), new((n + 63) // 64)
    st, off, tot = new(6), new((n + _lib.PARTITION_BLOCK - 1) // _lib.PARTITION_BLOCK), new(2)
    so, co = new(n), new(n)

    def run():
        codes = (L.esr_emit_decide(p(e), n, k_val, p(flags), p(st), 0, sp), L.esr_flags_pack(p(flags), n, p(words), sp),
                 L.esr_flag_scan_bits(p(words), n, p(off), p(tot), sp),
                 L.esr_index_partition_bits(p(rows), p(words), p(off), n, p(so), p(co), sp))
        if any(codes):
            raise RuntimeError(f"entry points failed with codes {codes}")

    run()                                                    # warm-up, and the outputs against torch
    n_set = int(tot[0])
    keep = e.max(1)[0] > k_val
    equal = bool(torch.equal(so[:n_set], rows[keep]) and torch.equal(co[:n - n_set], rows[~keep]))
    del keep
    res = summary([[run_ms(run) for _ in range(repeats)] for _ in range(rounds)], n)
    res.update(k_val=k_val, set_share=round(n_set / n, 5), outputs_equal_torch=equal)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--rows", type=int, default=USER_RAYS)
    ap.add_argument("--share-rows", type=int, default=1 << 26)
    ap.add_argument("--old-certain", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("regroup_time.py measures on the GPU; none is visible")
    from esr_nerf_amd import regroup
    out = dict(repeats=a.repeats, rounds=a.rounds, module_default=regroup.DEFAULT_BATCH_SIZE, device=torch.cuda.get_device_name(0))
    if not a.kernels_only:
        out.update(loop_section(a))
        torch.cuda.empty_cache()
    out.update(partition_section(a))
    torch.cuda.empty_cache()
    out["resplit_kernels_rows"] = a.share_rows
    out["resplit_kernels"] = {str(sh): resplit_kernels_at(a.share_rows, sh, 2 * a.repeats, a.rounds) for sh in SHARES}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
