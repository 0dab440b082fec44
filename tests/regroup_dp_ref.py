"""Restatement in numpy of what the re-split under data parallelism adds to tests/regroup_ref.py (esr_nerf_amd/regroup.py
over csrc/regroup.hip): the packed flag words, the ranks' shares, the merge of the ranks' records -- and the worker that
tests/test_regroup_dp_host.py (gloo ranks on the CPU) and tests/test_gpu_regroup_dp.py (gloo ranks on the one GPU) start under
``torch.distributed.run``."""
import numpy as np

import regroup_ref as R


def n_words(n):
    return (n + 63) // 64


def pack(flags):
    """[n] bool / uint8 -> [ceil(n / 64)] uint64: bit b of word w is flag 64 w + b, bit 0 the least significant"""
    f = np.asarray(flags) != 0
    bits = np.zeros(64 * n_words(len(f)), np.uint64)
    bits[:len(f)] = f
    return (bits.reshape(-1, 64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


def unpack(words, n):
    w = np.asarray(words, np.uint64)
    return ((w[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(-1)[:n].astype(bool)


def ray_share(n, rank, world):
    w = n_words(n)
    return 64 * (w * rank // world), min(n, 64 * (w * (rank + 1) // world))


def merge_records(records):
    """records: dicts of R.stats -> one: counts added, minima and maxima by R.order_key"""
    out = dict(records[0])
    for r in records[1:]:
        for k in R.STAT_KEYS:
            if k.startswith("n_"):
                out[k] = out[k] + r[k]
            else:
                a, b = np.float32(out[k]), np.float32(r[k])
                first = R.order_key(a) <= R.order_key(b)
                out[k] = (a if first else b) if k.startswith("min") else (b if first else a)
    return out


def check_argument_codes(L):
    """The packed entry points of the loaded library ``L`` check their arguments on the host, with pointers that are never
    followed: n == 0 succeeds without touching a pointer, a negative n and a NULL or misaligned pointer are ESR_EINVAL, 2^31
    rows are ESR_ECAP.  (No call here passes every check, so nothing is launched.)"""
    import ctypes
    null, ok, odd = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    calls = {
        "decide": lambda n, e, w, s: L.esr_emit_decide_bits(e, n, 0.5, w, s, 1, null),
        "pack": lambda n, f, w, _: L.esr_flags_pack(f, n, w, null),
        "unpack": lambda n, f, w, _: L.esr_flags_unpack(w, n, f, null),
        "scan": lambda n, o, w, t: L.esr_flag_scan_bits(w, n, o, t, null),
        "partition": lambda n, r, w, o: L.esr_index_partition_bits(r, w, o, n, ok, ok, null),
        "merge": lambda n, p, o, _: L.esr_regroup_stats_merge(p, n, o, null),
    }
    for name, call in calls.items():
        for n, code in ((0, 0), (-1, -1), (1 << 31, -2), ((1 << 31) + 5, -2)):
            assert call(n, null, null, null) == code, (name, n)
            assert call(n, ok, ok, ok) == code, (name, n)
        for args in ((null, ok, ok), (ok, null, ok), (ok, odd, ok)):
            assert call(5, *args) == -1, (name, args)                  # (the second pointer is the words / the output record)
    decide, scan, part = L.esr_emit_decide_bits, L.esr_flag_scan_bits, L.esr_index_partition_bits
    assert decide(ok, 5, 0.5, ok, null, 1, null) == -1 and decide(ok, 5, 0.5, ok, odd, 1, null) == -1
    assert decide(ctypes.c_void_p(0x1002), 5, 0.5, ok, ok, 0, null) == -1
    assert scan(ok, 5, odd, ok, null) == -1 and scan(ok, 5, ok, odd, null) == -1
    assert scan(ok, 5, null, ok, null) == -1 and scan(ok, 5, ok, null, null) == -1
    assert part(odd, ok, ok, 5, ok, ok, null) == -1 and part(ok, ok, odd, 5, ok, ok, null) == -1
    assert part(ok, ok, ok, 5, null, null, null) == -1 and part(ok, ok, ok, 5, odd, ok, null) == -1
    assert part(ok, ok, ok, 5, ok, odd, null) == -1 and part(ok, ok, null, 5, ok, ok, null) == -1
    assert L.esr_regroup_stats_merge(odd, 2, ok, null) == -1


# ---- the worker ------------------------------------------------------------------------------------------------------------------
# argv: repository root, device ("cpu" / "cuda:0"), the parts to run (comma-separated: stub, fail, model)
WORKER = r'''
import os, sys
ROOT, DEVICE, PARTS = sys.argv[1], sys.argv[2], sys.argv[3].split(",")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.distributed as dist
import regroup_ref as R
import regroup_dp_ref as D
from esr_nerf_amd import regroup
from esr_nerf_amd.config import AttrDict
from esr_nerf_amd.data import RayGroupManager

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
WORLD = dist.group.WORLD
on_gpu = DEVICE != "cpu"
if on_gpu:
    torch.cuda.set_device(0)
K = 0.40575385
KEYS = ["rays_o", "rays_d", "viewdirs"]


class Stub:
    """eval_emit is a pure function of the rays it is given (rays_o[:, 0] carries a ray's original row into a table), so a
    ray's emission depends on neither its chunk nor its rank; every call's rows are recorded"""

    def __init__(self, table, fail=False):
        self.table, self.fail, self.rows, self.modes_seen = table, fail, [], []
        self.train(True)

    def forward_training(self, **kw):
        raise AssertionError("not called")

    def forward_finetune(self, **kw):
        raise AssertionError("not called")

    def train(self, mode=True, finetune=False):
        self.training = mode
        self.forward = self.forward_finetune if (mode and finetune) else self.forward_training
        return self

    def eval(self):
        return self.train(False)

    def mode(self):
        return "eval" if not self.training else "finetune" if self.forward == self.forward_finetune else "train"

    def eval_emit(self, rays_o, rays_d, viewdirs):
        assert rays_o.shape == rays_d.shape == viewdirs.shape and rays_o.device.type == torch.device(DEVICE).type
        self.modes_seen.append(self.mode())
        if self.fail:
            raise RuntimeError("eval_emit failed")
        rows = rays_o[:, 0].long()
        self.rows.append(rows.cpu())
        return self.table[rows]


class CameraStyle(RayGroupManager):
    """A sampler that holds no ray arrays, as a camera-defined set: regroup._chunk_rays asks camera_batch for its rays"""

    def __init__(self, cfg, data, *a, **kw):
        super().__init__(cfg, data, *a, **kw)
        self.cams, self.images, self.em_modes, self.white_bg = self.data, None, None, True
        del self.data


def _camera_batch(cams, images, em_modes, rows, white_bg, check_rows=True):
    return {k: cams[k][rows].to(DEVICE) for k in KEYS}


def samplers(n_u, n_c, seed, preload, camera):
    g = torch.Generator().manual_seed(seed)
    n = n_u + n_c
    perm = torch.randperm(n, generator=g)
    data = {"rays_o": torch.arange(n, dtype=torch.float32)[:, None].repeat(1, 3), "rays_d": torch.randn(n, 3, generator=g),
            "viewdirs": torch.randn(n, 3, generator=g)}
    cfg = AttrDict(system=dict(device=DEVICE, data_preload=preload))
    cls = CameraStyle if camera else RayGroupManager
    make = lambda r, w: cls(cfg, data, list(KEYS), 24, 8, 48, 16, perm[:n_u].clone(), perm[n_u:].clone(), rank=r, world=w)
    return make(rank, world), make(0, 1), perm[:n_u]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


if "stub" in PARTS or "fail" in PARTS:
    import esr_nerf_amd.camera as camera_module
    real_camera_batch = camera_module.camera_batch
    camera_module.camera_batch = _camera_batch
    #        name        n_u          n_c  preload  camera  batch_size
    CASES = [("edges",   5 * 64 + 37, 40,  "cuda",  False,  100),
             ("one_word", 59,         7,   "cuda",  False,  None),
             ("empty",   0,           9,   "cuda",  False,  None),
             ("cpu_home", 5 * 64 + 37, 40, "cpu",   False,  64),
             ("camera",  5 * 64 + 37, 40,  "cuda",  True,   130),
             ("all_clear", 200,       0,   "cuda",  False,  None)]
    for name, n_u, n_c, preload, camera, bs in CASES if "stub" in PARTS else []:
        k = 100.0 if name == "all_clear" else K
        table = torch.from_numpy(R.emission_case(n_u + n_c, K, 31, edges=True)).to(DEVICE)
        s, s1, u0 = samplers(n_u, n_c, 4, preload, camera)
        if name == "edges":                                           # the edge rows sit INSIDE the uncertain group
            e_u = table[u0.to(DEVICE)].cpu().numpy()
            k32 = np.float32(K)
            up, dn = np.nextafter(k32, np.float32(np.inf)), np.nextafter(k32, np.float32(-np.inf))
            m = np.fmax.reduce(e_u, axis=1)
            assert (m == k32).any() and (m == up).any() and (m == dn).any() and np.isnan(e_u).any(), name
        u1, c1 = s1.uncert_data_idxs.clone(), s1.cert_data_idxs.clone()
        stub1 = Stub(table)
        one = regroup.update_ray_groups(stub1, s1, k, batch_size=bs, verbose=False, return_emission=True)
        # the single-process run: chunks of exactly batch_size rays (they may start inside a word), the restatement's flags,
        # and the groups that filter makes of them
        size1 = regroup.DEFAULT_BATCH_SIZE if bs is None else bs
        assert [len(r) for r in stub1.rows] == [min(size1, n_u - a) for a in range(0, n_u, size1)], (name, [len(r) for r in stub1.rows])
        want1 = torch.from_numpy(R.decide(table[u0.to(DEVICE)].cpu().numpy(), np.float32(k)))
        assert one.flags.dtype == torch.bool and torch.equal(one.flags.cpu(), want1), name
        twin = RayGroupManager(AttrDict(system=dict(device="cpu", data_preload="cpu")), {k_: torch.zeros(n_u + n_c, 3) for k_ in KEYS},
                               list(KEYS), 24, 8, 48, 16, u1.cpu(), c1.cpu())
        twin.filter(want1)
        assert torch.equal(s1.uncert_data_idxs.cpu(), twin.uncert_data_idxs) and torch.equal(s1.cert_data_idxs.cpu(), twin.cert_data_idxs), name
        stub = Stub(table)
        rep = regroup.update_ray_groups(stub, s, k, batch_size=bs, verbose=False, return_emission=True, process_group=WORLD)
        assert stub.mode() == "train" and set(stub.modes_seen) <= {"eval"}, name
        # the groups, the batch starts, the report: those of the single-process run, exactly
        assert torch.equal(s.uncert_data_idxs, s1.uncert_data_idxs) and torch.equal(s.cert_data_idxs, s1.cert_data_idxs), name
        assert s.uncert_data_idxs.device == s1.uncert_data_idxs.device and s.uncert_data_idxs.dtype == torch.int64, name
        assert (s.uncert_batch_st, s.cert_batch_st) == (48, 16) == (s1.uncert_batch_st, s1.cert_batch_st), name
        assert (rep.uncertain_before, rep.certain_before, rep.uncertain_after, rep.certain_after) == \
            (one.uncertain_before, one.certain_before, one.uncertain_after, one.certain_after) == \
            (n_u, n_c, s.uncert_data_num, s.cert_data_num), name
        assert not R.same_stats(rep.stats, one.stats) and set(rep.stats) == set(R.STAT_KEYS), (name, rep.stats, one.stats)
        assert rep.flags.dtype == torch.bool and len(rep.flags) == n_u and torch.equal(rep.flags.cpu(), one.flags.cpu()), name
        want = R.decide(table[u0.to(DEVICE)].cpu().numpy(), np.float32(k))
        assert np.array_equal(rep.flags.cpu().numpy(), want), name
        assert name in ("empty", "all_clear") or 0 < rep.uncertain_after < n_u, name
        # this rank evaluated its own share and nothing else, in chunks that start on a word
        lo, hi = regroup.ray_share(n_u, rank, world)
        assert (lo, hi) == D.ray_share(n_u, rank, world)
        size = (regroup.DEFAULT_BATCH_SIZE if bs is None else bs + 63) // 64 * 64
        assert [len(r) for r in stub.rows] == [min(size, hi - a) for a in range(lo, hi, size)], (name, [len(r) for r in stub.rows])
        seen = torch.cat(stub.rows) if stub.rows else torch.zeros(0, dtype=torch.int64)
        assert torch.equal(seen, u0[lo:hi]), name
        # return_emission: this rank's own rows, NaN elsewhere
        own = torch.zeros(n_u, dtype=torch.bool)
        own[lo:hi] = True
        e, e1 = rep.emission.cpu(), one.emission.cpu()
        assert torch.equal(bits(e[own]), bits(e1[own])) and bool(torch.isnan(e[~own]).all()), name
        dist.barrier()
    if "fail" in PARTS:
        # eval_emit raises on rank 1 only: EVERY rank raises, every renderer has its mode back, no group has changed
        table = torch.from_numpy(R.emission_case(400, K, 31)).to(DEVICE)
        for mode in ("train", "finetune", "eval"):
            s, _, u0 = samplers(5 * 64 + 37, 43, 4, "cuda", False)
            c0 = s.cert_data_idxs.clone()
            stub = Stub(table, fail=(rank == 1))
            if mode != "train":
                stub.train(True, finetune=True) if mode == "finetune" else stub.eval()
            try:
                regroup.update_ray_groups(stub, s, K, batch_size=128, verbose=False, process_group=WORLD)
                raised = None
            except regroup.RemoteFailure as e:
                raised = "remote"
            except RuntimeError as e:
                raised = "own" if "eval_emit failed" in str(e) else repr(e)
            assert raised == ("own" if rank == 1 else "remote"), (rank, raised)
            assert stub.mode() == mode and set(stub.modes_seen) <= {"eval"}
            assert torch.equal(s.uncert_data_idxs.cpu(), u0) and torch.equal(s.cert_data_idxs, c0)
        # ... and the next re-split of the same group works
        s, s1, _ = samplers(5 * 64 + 37, 43, 4, "cuda", False)
        regroup.update_ray_groups(Stub(table), s, K, verbose=False, process_group=WORLD)
        regroup.update_ray_groups(Stub(table), s1, K, verbose=False)
        assert torch.equal(s.uncert_data_idxs, s1.uncert_data_idxs) and torch.equal(s.cert_data_idxs, s1.cert_data_idxs)
        # a process group of another size than the sampler's world is refused before anything runs
        odd = RayGroupManager(AttrDict(system=dict(device=DEVICE, data_preload="cuda")),
                              {k: torch.zeros(8, 3) for k in KEYS}, list(KEYS), 4, 4, rank=rank, world=world + 1)
        try:
            regroup.update_ray_groups(Stub(table), odd, K, verbose=False, process_group=WORLD)
            raise AssertionError("not refused")
        except ValueError as e:
            assert "process group" in str(e)
    camera_module.camera_batch = real_camera_batch

if "model" in PARTS:
    # the real g16 model.  eval_emit's compositing sums by atomics, so a ray's emission may move in its last bits with the
    # chunking: k_val is put into the widest gap of the per-ray maxima between their quartiles, which must be wide
    from conftest import load_npz
    from esr_nerf_amd.camera import CameraRayGroupManager, Cameras
    from esr_nerf_amd.config import lts_cfg
    from esr_nerf_amd.esrnerf import ESRNeRF
    from esr_nerf_amd.synthetic import slab_scene
    from esr_nerf_amd.trainer import LtsStep
    import camera_ref as CR
    H, W_ = 48, 40
    MKEYS = ["rgbs", "rays_o", "rays_d", "viewdirs", "em_modes"]
    sc = slab_scene("g16", s_val=60.0, oblique=True, n_rays=H * W_, seed=0, mask="prune")
    torch.manual_seed(0); np.random.seed(0)
    cfg = lts_cfg("cuda:0", num_2ndrays=8, num_ltspts=12)
    cfg.system["data_preload"] = "cuda"
    m = ESRNeRF(cfg, sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max, sc.mask_alpha_init,
                sc.mask_density, sc.s_val, sc.num_voxels)
    m.load_state_dict({k: torch.from_numpy(v).cuda() for k, v in load_npz("lts_g16_params.npz").items()})
    m.s_val = 60.0
    m.train()
    perm = torch.randperm(H * W_, generator=torch.Generator().manual_seed(5))

    def manager(r, w):
        return RayGroupManager(cfg, {k: sc.batch[k] for k in MKEYS}, list(MKEYS), 128, 128, uncert_data_idxs=perm[:1500].clone(),
                               cert_data_idxs=perm[1500:].clone(), rank=r, world=w)

    def gap_k(emission):
        """(k_val, gap): the midpoint of the widest gap between consecutive sorted per-ray maxima inside the quartiles"""
        mx = np.sort(emission.max(1)[0].cpu().numpy().astype(np.float64))
        mid = mx[len(mx) // 4:3 * len(mx) // 4 + 1]
        i = int(np.argmax(np.diff(mid)))
        return float(np.float32(0.5 * (mid[i] + mid[i + 1]))), float(mid[i + 1] - mid[i])

    def share_k(emission):
        kg = torch.tensor(gap_k(emission), dtype=torch.float64)
        dist.broadcast(kg, 0)                                        # every rank takes rank 0's choice
        k_val, gap = float(kg[0]), float(kg[1])
        ulp = float(np.spacing(np.float32(k_val)))
        print(f"DPMODEL rank {rank}: k_val {k_val} gap {gap} = {gap / ulp:.0f} ulp", flush=True)
        assert gap > 1000 * ulp, (k_val, gap, ulp)                   # a condition on the input
        return k_val

    probe = regroup.update_ray_groups(m, manager(0, 1), 0.5, batch_size=500, verbose=False, return_emission=True)
    k_val = share_k(probe.emission)
    s, s1 = manager(rank, world), manager(0, 1)
    one = regroup.update_ray_groups(m, s1, k_val, batch_size=500, verbose=False)
    rep = regroup.update_ray_groups(m, s, k_val, batch_size=300, verbose=False, process_group=WORLD)
    assert m.training and not hasattr(m, "emit_color")
    assert torch.equal(rep.flags, one.flags) and 0.2 * 1500 < rep.uncertain_after < 0.8 * 1500, rep.uncertain_after
    assert torch.equal(s.uncert_data_idxs, s1.uncert_data_idxs) and torch.equal(s.cert_data_idxs, s1.cert_data_idxs)
    assert (rep.stats["n_set"], rep.stats["n_clear"], rep.stats["n_nan"]) == (one.stats["n_set"], one.stats["n_clear"], 0)

    # a camera-defined set
    eyes = [(0.3, -0.2, 2.4), (1.2, 0.8, 2.0), (-0.9, 0.5, 2.2)]
    poses = np.stack([CR.look_at_cv(e, (0.05, -0.05, 0.0)) for e in eyes])
    Kmat = np.array([[40.0, 0.0, 24.0], [0.0, 40.0, 20.0], [0.0, 0.0, 1.0]])
    cams = Cameras.from_intrinsics(poses, Kmat, 48, 40, device=torch.device("cuda:0"))
    nc = cams.n_rays
    g = torch.Generator().manual_seed(9)
    cperm = torch.randperm(nc, generator=g)
    images = torch.randint(0, 256, (nc, 4), generator=g, dtype=torch.uint8)
    ccfg = AttrDict(system=dict(device="cuda:0", data_preload="cuda"), data=dict(white_bg=True))

    def cam_manager(r, w):
        return CameraRayGroupManager(ccfg, cams, images, torch.tensor([0, 1, 0]), list(KEYS), 64, 64,
                                     uncert_data_idxs=cperm[:nc - 700].clone(), cert_data_idxs=cperm[nc - 700:].clone(), rank=r, world=w)

    probe = regroup.update_ray_groups(m, cam_manager(0, 1), 0.5, batch_size=2000, verbose=False, return_emission=True)
    k_cam = share_k(probe.emission)
    cs, cs1 = cam_manager(rank, world), cam_manager(0, 1)
    one = regroup.update_ray_groups(m, cs1, k_cam, batch_size=2000, verbose=False)
    rep = regroup.update_ray_groups(m, cs, k_cam, batch_size=1000, verbose=False, process_group=WORLD)
    assert torch.equal(rep.flags, one.flags) and 0 < rep.uncertain_after < nc - 700
    assert torch.equal(cs.uncert_data_idxs, cs1.uncert_data_idxs) and torch.equal(cs.cert_data_idxs, cs1.cert_data_idxs)

    # the engine trains after the re-split: one data-parallel PDRA step on the regrouped sampler's next batch
    m.pdra_mode = True
    step = LtsStep(m, cfg.app.trainer, stage="pdra", process_group=WORLD)
    batch = s.sample()
    count = torch.tensor([len(batch["rays_o"])])
    dist.all_reduce(count)
    torch.manual_seed(100 + rank); np.random.seed(100 + rank)
    loss, G, _ = step.forward_loss_backward(batch, 60.0, global_rays=int(count), entropy_owner=(rank == world - 1))
    torch.cuda.synchronize()
    step.close()
    losses = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(losses, torch.tensor([float(loss)], dtype=torch.float64))
    assert np.isfinite(float(loss)) and all(float(l) == float(losses[0]) for l in losses), losses
    assert G and all(bool(torch.isfinite(v).all()) for v in G.values())

dist.barrier()
print(f"DPREGROUP rank {rank} of {world} ok: {','.join(PARTS)}", flush=True)
dist.destroy_process_group()
'''
