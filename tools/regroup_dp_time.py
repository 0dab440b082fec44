"""Times of PDRA's re-split on packed flag words as a rank under data parallelism runs it (esr_nerf_amd/csrc/regroup.hip), and a
two-rank flow rehearsal of ``update_ray_groups(..., process_group=)``.

    python tools/regroup_dp_time.py [--rows 67108864] [--repeats 10] [--rounds 3] [--out FILE]

(a) ``--rows`` rows (2^26: 100 views of 800 x 800 are 64 M rays) at three set shares (1 %, 50 %, 99 %: emission uniform in
    [0, 1), ``k_val = (1 - share)^(1/3)``): ``esr_emit_decide_bits`` + ``esr_flag_scan_bits`` + ``esr_index_partition_bits``, and
    scan + partition alone.  Device events around each form, one warm-up, ``--repeats`` runs per round and their median,
    ``--rounds`` rounds alternating the forms; ``ms`` is the median of the rounds' medians, ``spread`` the range of the rounds'
    medians over it.  The outputs are compared with torch's boolean indexing first.  (profiles/regroup_dp_time.json is the
    record of this tool at ABI 38, when it timed the byte scan and partition beside the packed ones: the comparison that
    removed them.  tools/regroup_time.py times the single-process form, decide into bytes + pack + scan + partition.)
(b) FLOW REHEARSAL, not a scaling measurement: a re-split of the g16 slab model's rays by two ranks that SHARE the one GPU
    over gloo (as ``ESR_BENCH_REHEARSAL`` does for bench.py; RCCL refuses two ranks per device) against the single-process
    re-split in the same setting.  It shows that the flow runs and what its fixed costs are on one card; both ranks compete
    for the same device and gloo stages through the host, so it says nothing about two GPUs.
One JSON line.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHARES = (0.01, 0.5, 0.99)
REHEARSAL_RAYS, REHEARSAL_PORT = 1 << 18, 29571


def run_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(per_round):
    med = [float(np.median(r)) for r in per_round]
    m = float(np.median(med))
    return dict(ms_round_medians=[round(v, 4) for v in med], ms=round(m, 4), spread=round((max(med) - min(med)) / m, 4))


def kernels_at(n, share, repeats, rounds):
    from esr_nerf_amd import _lib
    dev = torch.device("cuda:0")
    L, sp, p = _lib.lib(), _lib.stream_ptr(dev), _lib.ptr
    g = torch.Generator(device=dev).manual_seed(int(share * 100))
    e = torch.rand(n, 3, device=dev, generator=g)
    k_val = float((1.0 - share) ** (1.0 / 3.0))
    rows = torch.randperm(n, device=dev, generator=g)
    n_tiles = (n + _lib.PARTITION_BLOCK - 1) // _lib.PARTITION_BLOCK
    new = lambda m: torch.empty(m, dtype=torch.int64, device=dev)
    words, st, off, tot, so, co = new((n + 63) // 64), new(6), new(n_tiles), new(2), new(n), new(n)

    def check(code):
        if code:
            raise RuntimeError(f"entry point failed with code {code}")

    def decide():
        check(L.esr_emit_decide_bits(p(e), n, k_val, p(words), p(st), 0, sp))

    def scan_partition():
        check(L.esr_flag_scan_bits(p(words), n, p(off), p(tot), sp))
        check(L.esr_index_partition_bits(p(rows), p(words), p(off), n, p(so), p(co), sp))

    variants = {"packed_decide_scan_partition": lambda: (decide(), scan_partition()), "packed_scan_partition": scan_partition}
    decide()                                                 # warm-up, and the outputs against torch
    scan_partition()
    n_set = int(tot[0])
    keep = e.max(1)[0] > k_val
    equal = bool(torch.equal(so[:n_set], rows[keep]) and torch.equal(co[:n - n_set], rows[~keep]))
    del keep
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append([run_ms(fn) for _ in range(repeats)])
    res = {k: summary(v) for k, v in times.items()}
    res.update(k_val=k_val, set_share=round(n_set / n, 5), outputs_equal_torch=equal)
    return res


def rehearsal_resplit(repeats, process_group=None, rank=0, world=1):
    """ms of ``update_ray_groups`` on the g16 slab model's rays (all uncertain, k_val the median per-ray maximum)"""
    from esr_nerf_amd import regroup
    from esr_nerf_amd.config import lts_cfg
    from esr_nerf_amd.data import RayGroupManager
    from esr_nerf_amd.esrnerf import ESRNeRF
    from esr_nerf_amd.synthetic import init_slab_model, slab_scene
    n = REHEARSAL_RAYS
    sc = slab_scene("g16", s_val=60.0, oblique=True, n_rays=n, seed=0)
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = lts_cfg("cuda:0", num_2ndrays=8, num_ltspts=12)
    cfg.system["data_preload"] = "cuda"
    m = init_slab_model(ESRNeRF(cfg, sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max,
                                sc.mask_alpha_init, sc.mask_density, sc.s_val, sc.num_voxels), sc)
    m.s_val = sc.s_val
    m.train()
    keys = ["rays_o", "rays_d", "viewdirs", "em_modes"]
    s = RayGroupManager(cfg, {k: sc.batch[k] for k in keys}, keys, 128, 128,
                        uncert_data_idxs=torch.randperm(n, generator=torch.Generator().manual_seed(0)), rank=rank, world=world)
    base = s.uncert_data_idxs
    one = RayGroupManager(cfg, {k: sc.batch[k] for k in keys}, keys, 128, 128, uncert_data_idxs=base.cpu())
    k_val = float(regroup.update_ray_groups(m, one, 0.0, verbose=False, return_emission=True).emission.max(1)[0].median())
    if process_group is not None:                            # every rank takes rank 0's k_val
        import torch.distributed as dist
        kt = torch.tensor([k_val], dtype=torch.float64)
        dist.broadcast(kt, 0)
        k_val = float(kt)
    ms, kept = [], None
    for i in range(repeats + 1):                             # (the first run is the warm-up)
        s.uncert_data_idxs, s.cert_data_idxs = base, base[:0]
        t = run_ms(lambda: regroup.update_ray_groups(m, s, k_val, verbose=False, process_group=process_group))
        kept = s.uncert_data_num
        if i:
            ms.append(t)
    return dict(ms=round(float(np.median(ms)), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), rays=n, k_val=k_val,
                uncertain_after=kept)


def rank_main(repeats):
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    res = rehearsal_resplit(repeats, dist.group.WORLD, rank, world)
    worst = torch.tensor([res["ms"]], dtype=torch.float64)
    dist.all_reduce(worst, op=dist.ReduceOp.MAX)             # a re-split ends when its slowest rank ends
    if rank == 0:
        print("REHEARSAL " + json.dumps(dict(res, ms_max_over_ranks=round(float(worst), 3), ranks=world)), flush=True)
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 26)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-rehearsal", action="store_true")
    ap.add_argument("--rank-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("regroup_dp_time.py measures on the GPU; none is visible")
    if a.rank_worker:
        return rank_main(a.repeats)
    out = dict(rows=a.rows, repeats=a.repeats, rounds=a.rounds, device=torch.cuda.get_device_name(0),
               shares={str(s): kernels_at(a.rows, s, a.repeats, a.rounds) for s in SHARES})
    torch.cuda.empty_cache()
    if not a.no_rehearsal:
        single = rehearsal_resplit(a.repeats)
        torch.cuda.synchronize()
        child = subprocess.run(
            [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
             "--master-port", str(REHEARSAL_PORT), os.path.abspath(__file__), "--rank-worker", "--repeats", str(a.repeats)],
            env=dict(os.environ, OMP_NUM_THREADS="2"), capture_output=True, text=True, timeout=600)
        lines = [l for l in child.stdout.splitlines() if l.startswith("REHEARSAL ")]
        if child.returncode != 0 or not lines:
            sys.exit("the two-rank rehearsal failed:\n" + child.stdout[-2000:] + child.stderr[-3000:])
        out["rehearsal"] = dict(
            note="FLOW REHEARSAL: two ranks share ONE GPU over gloo (host-staged); not a scaling measurement",
            single_process=single, two_ranks_one_gpu_gloo=json.loads(lines[-1][len("REHEARSAL "):]))
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
