"""PDRA's ray re-split on the MI355X (esr_nerf_amd/regroup.py over csrc/regroup.hip): ``esr_emit_decide``, and
``esr_flags_pack`` -> ``esr_flag_scan_bits`` -> ``esr_index_partition_bits`` on packed words, through the C ABI against the
numpy restatements tests/regroup_ref.py and tests/regroup_dp_ref.py and torch's own indexing, exact, with guards and shifted
pointers; ``update_ray_groups`` on the reference's recorded emission (tests/golden/
lts_g16_evals*.npz), on a progressive sequence against the CPU oracle outside its decision band, on a camera-defined set, and
in front of a PDRA training step."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import camera_ref as CR
import regroup_dp_ref as D
import regroup_ref as R
from conftest import load_npz, rel_err

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
G = 64                                      # guard elements either side of every output
SIZES = [0, 1, 63, 64, 65, 2047, 2048, 2049, 100003]
K_FULL, K_PRUNE = 0.40575385, 0.33619818    # midpoints of the widest gaps of the recorded per-ray maxima (0.34 and 0.67 wide)
BAND = 1e-4                                 # the fixtures' tolerance, relative to the largest emission
BAND_CAP = 32


def _lib():
    from esr_nerf_amd import _lib as L
    return L


def _p(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def _stream():
    return _lib().stream_ptr(DEV)


# ---- esr_emit_decide -----------------------------------------------------------------------------------------------------------
def _decide_abi(e, k, cuts=()):
    """One call (or one per chunk, accumulating) with the flags pointer one byte off a guarded buffer -> (flags, stats dict,
    raw bytes of every output buffer)"""
    L = _lib()
    n = len(e)
    ed = torch.from_numpy(e).to(DEV)
    e0 = ed.clone()
    fbuf = torch.full((n + 2 * G + 1,), 0xA5, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((6 + 2 * G,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    edges = [0, *cuts, n]
    first = True
    for a, b in zip(edges[:-1], edges[1:]):
        code = L.lib().esr_emit_decide(_p(ed, 12 * a), b - a, float(k), _p(fbuf, G + 1 + a), _p(sbuf, 8 * G), 0 if first else 1,
                                       _stream())
        assert code == 0
        first = first and b == a               # (an empty chunk touches nothing: the record starts with the first ray)
    torch.cuda.synchronize()
    assert torch.equal(ed.view(torch.int32), e0.view(torch.int32))                 # (bits: the inputs hold NaNs)
    fb, sb = fbuf.cpu().numpy(), sbuf.cpu().numpy()
    assert (fb[:G + 1] == 0xA5).all() and (fb[G + 1 + n:] == 0xA5).all()
    assert (sb[:G] == 0x5A5A5A5A5A5A5A5A).all() and (sb[G + 6:] == 0x5A5A5A5A5A5A5A5A).all()
    rec = L.EsrRegroupStats.from_buffer_copy(sb[G:G + 6].tobytes())
    return fb[G + 1:G + 1 + n], {k_: getattr(rec, k_) for k_ in R.STAT_KEYS}, (fb.tobytes(), sb.tobytes())


@pytest.mark.parametrize("n", SIZES)
def test_decision_and_statistics_are_bit_equal_to_the_restatement_and_torch(n):
    for k in (K_FULL, 0.0):
        k32 = float(np.float32(k))
        e = R.emission_case(n, k32, 100 + n)
        flags, stats, raw = _decide_abi(e, k32)
        if n == 0:
            assert raw[1] == np.full(6 + 2 * G, 0x5A5A5A5A5A5A5A5A, np.int64).tobytes()      # n == 0 touches nothing
            continue
        want = R.decide(e, k32)
        assert set(np.unique(flags)) <= {0, 1}
        assert np.array_equal(flags.astype(bool), want)
        assert np.array_equal(want, (torch.max(torch.from_numpy(e), dim=-1)[0] > k32).numpy())          # pdra.py:911
        assert not R.same_stats(stats, R.stats(e, want)), (stats, R.stats(e, want))
        # three accumulated chunk calls equal one call; two runs are byte-identical
        cuts = (-(-n // 3), -(-2 * n // 3))
        flags3, stats3, _ = _decide_abi(e, k32, cuts)
        assert np.array_equal(flags3, flags) and not R.same_stats(stats3, stats)
        assert _decide_abi(e, k32)[2] == raw


def test_decide_wrapper_merges_chunks_into_one_record():
    from esr_nerf_amd import regroup
    e = R.emission_case(5000, K_FULL, 3)
    ed = torch.from_numpy(e).to(DEV)
    flags, stats = regroup.decide(ed, K_FULL)
    one = regroup.read_stats(stats)
    buf, st = torch.empty(5000, dtype=torch.bool, device=DEV), None
    for a in range(0, 5000, 1300):
        _, st = regroup.decide(ed[a:a + 1300], K_FULL, buf[a:a + 1300], st)
    assert torch.equal(buf, flags) and flags.dtype == torch.bool
    three = regroup.read_stats(st)
    want = R.stats(e, R.decide(e, np.float32(K_FULL)))
    assert not R.same_stats(one, want) and not R.same_stats(three, want)
    _, empty = regroup.decide(torch.empty(0, 3, device=DEV), K_FULL)
    assert not R.same_stats(regroup.read_stats(empty), R.stats(np.zeros((0, 3), np.float32), np.zeros(0, bool)))


# ---- esr_flags_pack, esr_flags_unpack, esr_flag_scan_bits, esr_index_partition_bits -----------------------------------------------
def _partition_sizes():
    L = _lib()
    pb, st = L.PARTITION_BLOCK, L.PARTITION_SCAN_TILE
    assert (pb, st) == (1024, 1024)
    # around one and two tiles; a ragged last tile and a ragged last word; a second trip of the one-block scan, twice
    return sorted(set(SIZES + [pb * k + d for k in (1, 2) for d in (-1, 0, 1)] + [4 * pb + 37, st * pb + 70000, (st + 1) * pb + 1]))


PARTITION_SIZES = sorted(set(SIZES + [1023, 1024, 1025, 2047, 2048, 2049, 4096 + 37, 1024 * 1024 + 70000, 1025 * 1024 + 1]))
GUARD = -0x0123456789ABCDEF


def _patterns(n, seed):
    p = R.flag_patterns(n, seed)
    p["random_50"] = np.random.default_rng(seed + 1).random(n) < 0.5
    return p


def _guarded(n, fill=GUARD, dtype=torch.int64, shift=1):
    """A buffer with G guard elements in front of and behind n elements that start `shift` elements further in (so an int64
    output sits 8 bytes off the allocation's alignment) -> (buffer, byte offset of the output, check(name) -> the output)"""
    buf = torch.full((n + 2 * G + shift,), fill, dtype=dtype, device=DEV)
    lo = G + shift

    def check(name):
        assert bool((buf[:lo] == fill).all()) and bool((buf[lo + n:] == fill).all()), name
        return buf[lo:lo + n]

    return buf, lo * buf.element_size(), check


@pytest.mark.parametrize("n", PARTITION_SIZES)
def test_scan_and_partition_equal_boolean_indexing(n):
    """pack -> scan -> partition on words against numpy and torch's boolean indexing"""
    L = _lib()
    lib = L.lib()
    assert PARTITION_SIZES == _partition_sizes()
    pb = L.PARTITION_BLOCK
    nw, n_tiles = D.n_words(n), -(-n // pb)
    assert n < 1024 * 1024 or n_tiles > L.PARTITION_SCAN_TILE         # the two largest: a second trip of the one-block scan
    rng = np.random.default_rng(n)
    rows_h = rng.integers(0, 1 << 62, size=n, dtype=np.int64)
    rows_h[::3] += 1 << 40
    assert n == 0 or rows_h.max() > 1 << 40
    rows_buf = torch.zeros(n + 1, dtype=torch.int64, device=DEV)      # the rows start 8 bytes into their allocation
    rows = rows_buf[1:]
    rows.copy_(torch.from_numpy(rows_h))
    rows0 = rows.clone()
    for name, f in _patterns(n, n + 1).items():
        fh = f.astype(np.uint8)
        fh[f & (np.arange(n) % 5 == 0)] = 255                        # any non-zero byte is a set flag
        fbuf = torch.zeros(n + 1, dtype=torch.uint8, device=DEV)
        flags = fbuf[1:]                                             # (bytes at an odd address)
        flags.copy_(torch.from_numpy(fh))
        flags0 = flags.clone()
        n_set = int(f.sum())
        want_words = D.pack(f)
        wbuf, woff, wcheck = _guarded(nw)
        ubuf, uoff, ucheck = _guarded(n, 0xA5, torch.uint8)
        obuf, ooff, ocheck = _guarded(n_tiles)
        tbuf, toff, tcheck = _guarded(2)
        sbuf, soff, scheck = _guarded(n_set)
        clear_buf = torch.full((3 + n - n_set + G,), GUARD, dtype=torch.int64, device=DEV)     # clear_out in its middle
        assert lib.esr_flags_pack(_p(flags), n, _p(wbuf, woff), _stream()) == 0
        assert lib.esr_flags_unpack(_p(wbuf, woff), n, _p(ubuf, uoff), _stream()) == 0
        assert lib.esr_flag_scan_bits(_p(wbuf, woff), n, _p(obuf, ooff), _p(tbuf, toff), _stream()) == 0
        assert lib.esr_index_partition_bits(_p(rows), _p(wbuf, woff), _p(obuf, ooff), n, _p(sbuf, soff), _p(clear_buf, 24),
                                            _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(rows, rows0) and torch.equal(flags, flags0), name
        if n == 0:                                                   # n == 0 touches nothing
            assert all(bool((t == GUARD).all()) for t in (wbuf, obuf, tbuf, sbuf, clear_buf)) and bool((ubuf == 0xA5).all()), name
            continue
        # pack: whole words, the tail of the last one clear, guards untouched (also after the scan and the partition read them)
        words = wcheck(name)
        assert np.array_equal(words.cpu().numpy().view(np.uint64), want_words), name
        if n % 64:
            assert int(want_words[-1]) >> (n % 64) == 0 and int(words[-1].cpu().numpy().view(np.uint64)) >> (n % 64) == 0, name
        # unpack: exactly 0 or 1, the round trip
        assert np.array_equal(ucheck(name).cpu().numpy(), f.astype(np.uint8)), name
        # scan on words == numpy
        per_tile = np.add.reduceat(f.astype(np.int64), np.arange(0, n, pb))
        want_off = np.concatenate([[0], np.cumsum(per_tile)[:-1]])
        assert np.array_equal(ocheck(name).cpu().numpy(), want_off), name
        assert tcheck(name).tolist() == [n_set, n - n_set], name
        # partition on words == boolean indexing
        fd = flags != 0
        assert torch.equal(fd, torch.from_numpy(f).to(DEV)), name
        assert torch.equal(scheck(name), rows[fd]), name
        assert torch.equal(clear_buf[3:3 + n - n_set], rows[~fd]), name
        assert bool((clear_buf[:3] == GUARD).all()) and bool((clear_buf[3 + n - n_set:] == GUARD).all()), name


def test_partition_wrapper_and_apply_flags_on_a_device_sampler():
    from esr_nerf_amd import regroup
    from esr_nerf_amd.config import AttrDict
    from esr_nerf_amd.data import RayGroupManager
    n_u, n_c = 5000, 333
    g = torch.Generator().manual_seed(2)
    perm = torch.randperm(n_u + n_c, generator=g)
    data = {k: torch.randn(n_u + n_c, 3, generator=g) for k in ("rays_o", "rays_d", "viewdirs")}
    cfg = AttrDict(system=dict(device="cuda:0", data_preload="cuda"))
    for name, f in R.flag_patterns(n_u, 5).items():
        flags = torch.from_numpy(f).to(DEV)
        a, b = (RayGroupManager(cfg, data, list(data), 24, 8, 48, 16, perm[:n_u], perm[n_u:]) for _ in range(2))
        a.filter(flags)
        assert regroup.apply_flags(b, flags) is None
        assert torch.equal(a.uncert_data_idxs, b.uncert_data_idxs) and torch.equal(a.cert_data_idxs, b.cert_data_idxs), name
        assert b.uncert_data_idxs.is_cuda and b.uncert_data_idxs.is_contiguous() and b.cert_data_idxs.is_contiguous()
        assert (b.uncert_batch_st, b.cert_batch_st) == (48, 16)
        s, c = regroup.partition(perm[:n_u].to(DEV), flags)
        assert torch.equal(s, a.uncert_data_idxs) and torch.equal(c, a.cert_data_idxs[n_c:]), name
    # uint8 flags: any non-zero byte is a set flag
    f8 = torch.from_numpy((np.random.default_rng(7).random(n_u) < 0.5).astype(np.uint8))
    f8[(f8 != 0) & (torch.arange(n_u) % 3 == 0)] = 2
    f8[(f8 != 0) & (torch.arange(n_u) % 3 == 1)] = 255
    assert {0, 1, 2, 255} == set(f8.unique().tolist())
    rows, flags = perm[:n_u].to(DEV), f8.to(DEV)
    s, c = regroup.partition(rows, flags)
    assert torch.equal(s, rows[flags != 0]) and torch.equal(c, rows[flags == 0])
    b = RayGroupManager(cfg, data, list(data), 24, 8, 48, 16, perm[:n_u], perm[n_u:])
    old_c = b.cert_data_idxs.clone()
    assert regroup.apply_flags(b, flags) is None
    assert torch.equal(b.uncert_data_idxs, rows[flags != 0]) and torch.equal(b.cert_data_idxs, torch.cat([old_c, rows[flags == 0]]))


# ---- update_ray_groups -----------------------------------------------------------------------------------------------------------
H, W = 48, 40
KEYS = ["rgbs", "rays_o", "rays_d", "viewdirs", "em_modes"]


def _sfx(mask):
    return "" if mask == "full" else "_" + mask


def _model(sc):
    from esr_nerf_amd.config import lts_cfg
    from esr_nerf_amd.esrnerf import ESRNeRF
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = lts_cfg("cuda:0", num_2ndrays=8, num_ltspts=12)
    cfg.system["data_preload"] = "cuda"
    m = ESRNeRF(cfg, sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max, sc.mask_alpha_init,
                sc.mask_density, sc.s_val, sc.num_voxels)
    sd = {k: torch.from_numpy(v) for k, v in load_npz("lts_g16_params.npz").items()}
    m.load_state_dict({k: v.cuda() for k, v in sd.items()})
    m.s_val = 60.0
    m.train()
    return m, cfg


def _manager(cfg, batch, uncert, cert, bs=128):
    from esr_nerf_amd.data import RayGroupManager
    return RayGroupManager(cfg, {k: batch[k] for k in KEYS}, list(KEYS), bs, bs, uncert_data_idxs=uncert.clone(),
                           cert_data_idxs=cert.clone())


@pytest.mark.parametrize("batch_size", [None, 20])
@pytest.mark.parametrize("mask,k_val,n_keep", [("full", K_FULL, 36), ("prune", K_PRUNE, 29)])
def test_regrouping_the_recorded_rays_equals_the_references_decisions(mask, k_val, n_keep, batch_size):
    from esr_nerf_amd import regroup
    from esr_nerf_amd.synthetic import slab_scene
    rec = load_npz(f"lts_g16_evals{_sfx(mask)}.npz")["out/eval_emit"]
    want = rec.max(1) > np.float32(k_val)
    assert rec.shape == (48, 3) and int(want.sum()) == n_keep
    assert np.abs(rec.max(1) - np.float32(k_val)).min() > 0.15                   # the gap against the fixture tolerance 1e-4
    sc = slab_scene("g16", s_val=60.0, oblique=True, mask=mask)
    m, cfg = _model(sc)
    perm = torch.randperm(48, generator=torch.Generator().manual_seed(1))
    s = _manager(cfg, sc.batch, perm, torch.arange(0))
    rep = regroup.update_ray_groups(m, s, k_val, batch_size=batch_size, verbose=False, return_emission=True)
    assert m.training and not hasattr(m, "emit_color")
    assert rel_err(rep.emission, torch.from_numpy(rec)[perm]) < 1e-4
    w = torch.from_numpy(want)[perm]
    assert torch.equal(rep.flags.cpu(), w)
    assert (rep.uncertain_before, rep.certain_before, rep.uncertain_after, rep.certain_after) == (48, 0, n_keep, 48 - n_keep)
    assert torch.equal(s.uncert_data_idxs.cpu(), perm[w]) and torch.equal(s.cert_data_idxs.cpu(), perm[~w])
    assert (rep.stats["n_set"], rep.stats["n_clear"], rep.stats["n_nan"]) == (n_keep, 48 - n_keep, 0)


@functools.lru_cache(maxsize=None)
def _oracle_emission(mask):
    """lp.eval_emit of the CPU oracle on all 1920 rays of the scene, once per mask"""
    from esr_nerf_amd.config import lts_cfg
    from esr_nerf_amd.synthetic import slab_scene
    from oracle import fine_path as fp
    from oracle import lts_path as lp
    sc = slab_scene("g16", s_val=60.0, oblique=True, n_rays=H * W, seed=0, mask=mask)
    ccfg = lts_cfg("cpu", num_2ndrays=8, num_ltspts=12)
    c = fp.make_consts(ccfg.app.model, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max, sc.mask_alpha_init,
                       sc.mask_density, sc.near, sc.num_voxels)
    sd = {k: torch.from_numpy(v) for k, v in load_npz("lts_g16_params.npz").items()}
    P = fp.params_from_state_dict(sd, requires_grad=False)
    return sc, lp.eval_emit(P, c, sc.batch, 60.0)


def _clear_of_band(oracle_e, k_val):
    """[n] bool: rays the oracle puts outside |max_c - k_val| <= BAND * max(emission); asserts the cap on the rest"""
    m = oracle_e.max(1)[0]
    clear = (m - k_val).abs() > BAND * float(oracle_e.max())
    assert int((~clear).sum()) <= BAND_CAP, int((~clear).sum())
    return clear


@pytest.mark.parametrize("mask", ["full", "prune"])
def test_progressive_sequence_equals_filter_and_the_oracle_outside_its_band(mask):
    from esr_nerf_amd import regroup
    sc, oe = _oracle_emission(mask)
    m, cfg = _model(sc)
    perm = torch.randperm(H * W, generator=torch.Generator().manual_seed(5))
    s = _manager(cfg, sc.batch, perm[:1500], perm[1500:])
    for _ in range(3):
        s.sample()                                                   # batch starts that are not 0
    in_band = []
    for k_val in (0.3, 0.6, 0.705):
        clear_all = _clear_of_band(oe, k_val)                        # over all 1920 rays, before anything is compared
        in_band.append(int((~clear_all).sum()))
        u0, c0 = s.uncert_data_idxs.clone(), s.cert_data_idxs.clone()
        st0 = (s.uncert_batch_st, s.cert_batch_st)
        twin = _manager(cfg, sc.batch, u0, c0)
        big = _manager(cfg, sc.batch, u0, c0)
        rep = regroup.update_ray_groups(m, s, k_val, batch_size=500, verbose=False, return_emission=True)
        assert m.training
        # the state is filter's on the returned flags, exactly
        twin.filter(rep.flags)
        assert torch.equal(s.uncert_data_idxs, twin.uncert_data_idxs) and torch.equal(s.cert_data_idxs, twin.cert_data_idxs)
        assert (s.uncert_batch_st, s.cert_batch_st) == st0
        # the report is torch on the returned emission
        e = rep.emission.cpu()
        assert torch.equal(rep.flags.cpu(), torch.max(e, dim=-1)[0] > k_val)
        assert not R.same_stats(rep.stats, R.stats(e.numpy(), rep.flags.cpu().numpy()))
        assert (rep.uncertain_before, rep.certain_before) == (len(u0), len(c0))
        assert (rep.uncertain_after, rep.certain_after) == (int(rep.flags.sum()), len(c0) + len(u0) - int(rep.flags.sum()))
        # the oracle's decision on every ray outside its band
        rows = u0.cpu()
        want, clear = oe[rows].max(1)[0] > k_val, clear_all[rows]
        assert torch.equal(rep.flags.cpu()[clear], want[clear]), k_val
        assert rel_err(e, oe[rows]) < 1e-4
        # another chunk size decides the same outside the band
        rep2 = regroup.update_ray_groups(m, big, k_val, batch_size=4096, verbose=False)
        assert torch.equal(rep2.flags.cpu()[clear], rep.flags.cpu()[clear]), k_val
        print(f"{mask} k_val {k_val}: {rep.uncertain_before} -> {rep.uncertain_after} uncertain, oracle band holds "
              f"{in_band[-1]} of {H * W} rays, chunk 500 / 4096 differ on {int((rep2.flags != rep.flags).sum())}")
        assert 0 < rep.uncertain_after < rep.uncertain_before
    assert in_band == ([0, 0, 17] if mask == "full" else [0, 0, 12])


def _camera_set():
    eyes = [(0.3, -0.2, 2.4), (1.2, 0.8, 2.0), (-0.9, 0.5, 2.2)]
    poses = np.stack([CR.look_at_cv(e, (0.05, -0.05, 0.0)) for e in eyes])
    K = np.array([[40.0, 0.0, 24.0], [0.0, 40.0, 20.0], [0.0, 0.0, 1.0]])
    return poses, K, 48, 40


def test_camera_defined_set_regroups_like_the_same_rays_in_arrays():
    from esr_nerf_amd import regroup
    from esr_nerf_amd.camera import CameraRayGroupManager, Cameras, camera_rays
    from esr_nerf_amd.config import AttrDict
    from esr_nerf_amd.data import RayGroupManager
    from esr_nerf_amd.synthetic import slab_scene
    sc = slab_scene("g16", s_val=60.0, oblique=True, mask="prune")
    m, _ = _model(sc)
    poses, K, w, h = _camera_set()
    cams = Cameras.from_intrinsics(poses, K, w, h, device=DEV)
    n = cams.n_rays
    assert n == 3 * 48 * 40
    cfg = AttrDict(system=dict(device="cuda:0", data_preload="cuda"), data=dict(white_bg=True))
    g = torch.Generator().manual_seed(9)
    perm = torch.randperm(n, generator=g)
    n_u = n - 700
    images = torch.randint(0, 256, (n, 4), generator=g, dtype=torch.uint8)
    modes = torch.tensor([0, 1, 0])
    keys = ["rays_o", "rays_d", "viewdirs"]
    cs = CameraRayGroupManager(cfg, cams, images, modes, list(keys), 64, 64, uncert_data_idxs=perm[:n_u], cert_data_idxs=perm[n_u:])
    ro, rd, vd = camera_rays(cams)
    rs = RayGroupManager(cfg, dict(rays_o=ro, rays_d=rd, viewdirs=vd), list(keys), 64, 64, uncert_data_idxs=perm[:n_u],
                         cert_data_idxs=perm[n_u:])
    k_val = 0.5
    reps = []
    for s in (cs, rs):
        u0, c0 = s.uncert_data_idxs.clone(), s.cert_data_idxs.clone()
        rep = regroup.update_ray_groups(m, s, k_val, batch_size=2000, verbose=False, return_emission=True)
        # each state is consistent with its own flags
        assert torch.equal(s.uncert_data_idxs, u0[rep.flags]) and torch.equal(s.cert_data_idxs, torch.cat([c0, u0[~rep.flags]]))
        assert torch.equal(rep.flags, torch.max(rep.emission, dim=-1)[0] > k_val)
        reps.append(rep)
    a, b = reps
    e = b.emission
    clear = (e.max(1)[0] - k_val).abs() > BAND * float(e.max())
    n_band = int((~clear).sum())
    print(f"camera set: {a.uncertain_after} / {b.uncertain_after} of {n_u} stay uncertain, {n_band} rays in the band, "
          f"{int((a.flags != b.flags).sum())} flags differ")
    assert n_band <= BAND_CAP
    assert torch.equal(a.flags[clear], b.flags[clear])
    assert 0.05 * n_u < a.uncertain_after < 0.95 * n_u


def test_cpu_home_sampler_is_regrouped_through_pinned_chunks():
    """``data_preload: cpu``: the arrays and index vectors stay on the host, a chunk is gathered into pinned memory and
    uploaded, the decision runs on the device and the existing ``filter`` lines regroup"""
    from esr_nerf_amd import regroup
    sc, oe = _oracle_emission("full")
    m, cfg = _model(sc)
    perm = torch.randperm(H * W, generator=torch.Generator().manual_seed(5))
    dev_s = _manager(cfg, sc.batch, perm[:1500], perm[1500:])
    from esr_nerf_amd.config import AttrDict
    host_s = _manager(AttrDict(system=dict(device="cuda:0", data_preload="cpu")), sc.batch, perm[:1500], perm[1500:])
    assert host_s.home == "cpu" and not host_s.uncert_data_idxs.is_cuda and not host_s.data["rays_o"].is_cuda
    k_val = 0.6
    clear = _clear_of_band(oe, k_val)[perm[:1500]]
    a = regroup.update_ray_groups(m, dev_s, k_val, batch_size=700, verbose=False, return_emission=True)
    b = regroup.update_ray_groups(m, host_s, k_val, batch_size=700, verbose=False, return_emission=True)
    assert b.flags.is_cuda and rel_err(b.emission, a.emission) < 1e-5
    assert torch.equal(b.flags, torch.max(b.emission, dim=-1)[0] > k_val)
    assert torch.equal(a.flags.cpu()[clear], b.flags.cpu()[clear]) and not R.same_stats(b.stats, R.stats(b.emission.cpu().numpy(), b.flags.cpu().numpy()))
    f = b.flags.cpu()
    assert not host_s.uncert_data_idxs.is_cuda
    assert torch.equal(host_s.uncert_data_idxs, perm[:1500][f]) and torch.equal(host_s.cert_data_idxs, torch.cat([perm[1500:], perm[:1500][~f]]))


def test_the_engine_still_trains_after_a_resplit():
    """One PDRA step on a fixed batch with fixed draws after ``update_ray_groups`` against the same step on a model that
    never regrouped (the eval passes leave the engine's buffers at the re-split's chunk size)"""
    from esr_nerf_amd import regroup
    from esr_nerf_amd.synthetic import slab_scene
    from esr_nerf_amd.trainer import LtsStep
    sc = slab_scene("g16", s_val=60.0, oblique=True, n_rays=H * W, seed=0, mask="prune")
    n_b, R2, Pn = 256, 8, 12
    b = {k: v[:n_b].cuda() for k, v in sc.batch.items()}
    b["uncert_masks"] = (torch.arange(n_b) % 3 != 0).cuda()
    res, draws = {}, None
    for tag in ("fresh", "regrouped"):
        m, cfg = _model(sc)
        m.pdra_mode = True
        step = LtsStep(m, cfg.app.trainer, stage="pdra")
        if draws is None:
            step.forward_loss_backward(b, 60.0)                      # internal draws, to learn the survivor count
            m3 = m.last_counts["m3"]
            g = torch.Generator().manual_seed(1)
            draws = dict(idx=torch.randperm(m3, generator=g)[:Pn].cuda(), dirs=torch.randn(Pn, R2 + 1, 3, generator=g).cuda(),
                         noise_normal=torch.randn(m3, 3, generator=g).cuda(), noise_emit=torch.randn(m3, 3, generator=g).cuda())
        if tag == "regrouped":
            perm = torch.randperm(H * W, generator=torch.Generator().manual_seed(5))
            s = _manager(cfg, sc.batch, perm[:1500], perm[1500:])
            rep = regroup.update_ray_groups(m, s, 0.6, batch_size=700, verbose=False)
            assert 0 < rep.uncertain_after < 1500
            assert m.training and not hasattr(m, "emit_color")       # back in train mode
        loss, Gr, _ = step.forward_loss_backward(b, 60.0, draws=draws)
        res[tag] = (float(loss), {k: v.clone() for k, v in Gr.items()})
    (l0, g0), (l1, g1) = res["fresh"], res["regrouped"]
    assert np.isfinite(l0) and abs(l1 - l0) < 1e-5 * max(1.0, abs(l0)), (l0, l1)
    bad = {k: rel_err(g1[k], v) for k, v in g0.items()}
    bad = {k: e for k, e in bad.items() if not e < 2e-5}
    assert g0 and not bad, str(bad)
