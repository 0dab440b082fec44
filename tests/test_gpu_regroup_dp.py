"""PDRA's re-split under data parallelism on the MI355X (esr_nerf_amd/regroup.py over csrc/regroup.hip): the decision into
words and the merge of the ranks' records through the C ABI, exactly, against the numpy restatement tests/regroup_dp_ref.py
and the byte decision on the same emission, with guards and shifted pointers (pack, scan and partition on words:
tests/test_gpu_regroup.py); the wrappers on a device sampler; and
``update_ray_groups(..., process_group=)`` with two and three ranks on the one GPU over gloo (the worker of
tests/regroup_dp_ref.py) against the single-process byte path, with a stub renderer, the real g16 model, a camera-defined
set, and a data-parallel PDRA step after the re-split."""
import ctypes as C

import numpy as np
import pytest
import torch

import regroup_dp_ref as D
import regroup_ref as R
from test_regroup_dp_host import run_ranks, why

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
G = 64                                      # guard elements either side of every output
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 4096 + 37, 1024 * 1024 + 70000]      # the last: a second trip of the one-block scan,
K = 0.40575385                                                                 # a ragged last tile and a ragged last word
GUARD = -0x0123456789ABCDEF
PATTERNS = ("all_set", "all_clear", "alternating", "random_1", "random_50", "random_99")


def _lib():
    from esr_nerf_amd import _lib as L
    return L


def _p(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def _stream():
    return _lib().stream_ptr(DEV)


def _patterns(n, seed):
    p = R.flag_patterns(n, seed)
    p["random_50"] = np.random.default_rng(seed + 1).random(n) < 0.5
    return {k: p[k] for k in PATTERNS}


def _guarded(n, fill=GUARD, dtype=torch.int64, shift=1):
    """A buffer with G guard elements in front of and behind n elements that start `shift` elements further in (so an int64
    output sits 8 bytes off the allocation's alignment) -> (buffer, byte offset of the output, check(name) -> the output)"""
    buf = torch.full((n + 2 * G + shift,), fill, dtype=dtype, device=DEV)
    lo = G + shift

    def check(name):
        assert bool((buf[:lo] == fill).all()) and bool((buf[lo + n:] == fill).all()), name
        return buf[lo:lo + n]

    return buf, lo * buf.element_size(), check


def _rec_bytes(r):
    return bytes(_lib().EsrRegroupStats(*(int(r[k]) if k.startswith("n_") else float(r[k]) for k in R.STAT_KEYS)))


def _record(words6):
    rec = _lib().EsrRegroupStats.from_buffer_copy(words6.tobytes())
    return {k: getattr(rec, k) for k in R.STAT_KEYS}


@pytest.mark.parametrize("n", SIZES)
def test_decision_into_words_equals_the_byte_decision_and_its_statistics(n):
    lib = _lib().lib()
    nw = D.n_words(n)
    for k in (K, 0.0):
        k32 = float(np.float32(k))
        e = R.emission_case(n, k32, 100 + n)                         # (a channel equal to k_val, one ulp either side, NaN, +-inf)
        ed = torch.from_numpy(e).to(DEV)
        e0 = ed.clone()
        want = R.decide(e, k32)
        # the byte kernel on the same emission
        flags_b, stats_b = torch.empty(n, dtype=torch.uint8, device=DEV), torch.empty(6, dtype=torch.int64, device=DEV)
        assert lib.esr_emit_decide(_p(ed), n, k32, _p(flags_b), _p(stats_b), 0, _stream()) == 0
        # one call, and three accumulated chunks that start on words
        cut = lambda x: min(n, -(-x // 64) * 64)
        for cuts in ((), (cut(n // 3), cut(2 * n // 3))):
            wbuf, woff, wcheck = _guarded(nw)
            sbuf, soff, scheck = _guarded(6, 0x5A5A5A5A5A5A5A5A)
            edges, first = [0, *cuts, n], True
            for a, b in zip(edges[:-1], edges[1:]):
                assert a % 64 == 0 or a == b
                assert lib.esr_emit_decide_bits(_p(ed, 12 * a), b - a, k32, _p(wbuf, woff + a // 8), _p(sbuf, soff),
                                                0 if first else 1, _stream()) == 0
                first = first and b == a                             # (an empty chunk touches nothing)
            torch.cuda.synchronize()
            words = wcheck(cuts).cpu().numpy().view(np.uint64)
            assert np.array_equal(words, D.pack(want)) and np.array_equal(D.unpack(words, n), flags_b.cpu().numpy().astype(bool)), cuts
            if n % 64:
                assert int(words[-1]) >> (n % 64) == 0
            got = scheck(cuts).cpu().numpy()
            assert got.tobytes() == stats_b.cpu().numpy().tobytes(), (cuts, _record(got), _record(stats_b.cpu().numpy()))
            assert not R.same_stats(_record(got), R.stats(e, want)), cuts
        assert torch.equal(ed.view(torch.int32), e0.view(torch.int32))


@pytest.mark.parametrize("n_parts", [1, 2, 8, 70])
def test_records_are_merged_as_the_host_merges_them(n_parts):
    from esr_nerf_amd import regroup
    L = _lib()
    k = np.float32(K)
    rng = np.random.default_rng(n_parts)
    recs = []
    for p in range(n_parts):
        m = 0 if p % 3 == 1 else int(rng.integers(1, 200))           # an empty part: +inf / -inf in all its groups
        e = R.emission_case(m, k, 50 + p, edges=False) * np.float32(1 + p % 4) - np.float32(p % 2)
        f = R.decide(e, k)
        if p % 4 == 2:
            f = np.zeros(m, bool)                                    # a part without set rays
        recs.append(R.stats(e, f))
    host = b"".join(_rec_bytes(r) for r in recs)
    parts = torch.frombuffer(bytearray(host), dtype=torch.int64).to(DEV)
    parts0 = parts.clone()
    obuf, ooff, ocheck = _guarded(6)
    assert L.lib().esr_regroup_stats_merge(_p(parts), n_parts, _p(obuf, ooff), _stream()) == 0
    torch.cuda.synchronize()
    got = _record(ocheck(n_parts).cpu().numpy())
    assert torch.equal(parts, parts0)
    assert not R.same_stats(got, D.merge_records(recs)), (got, D.merge_records(recs))
    want = None
    for r in recs:
        want = regroup._merge(want, {key: (int(r[key]) if key.startswith("n_") else float(r[key])) for key in R.STAT_KEYS})
    assert all(got[key] == want[key] for key in R.STAT_KEYS), (got, want)
    # `out` may be one of the parts; the wrapper takes the records at the front of an int64 vector
    regroup.merge_stats(parts, n_parts, parts)
    torch.cuda.synchronize()
    assert not R.same_stats(_record(parts[:6].cpu().numpy()), got) and torch.equal(parts[6:], parts0[6:])
    # the total order of the zeros: -0.0 is the minimum, +0.0 the maximum, whichever part holds which
    z = [dict(recs[0], min_all=np.float32(a), max_all=np.float32(b)) for a, b in ((0.0, -0.0), (-0.0, 0.0))]
    zp = torch.frombuffer(bytearray(b"".join(_rec_bytes(r) for r in z)), dtype=torch.int64).to(DEV)
    regroup.merge_stats(zp, 2, zp)
    torch.cuda.synchronize()
    zr = _record(zp[:6].cpu().numpy())
    assert np.signbit(np.float32(zr["min_all"])) and not np.signbit(np.float32(zr["max_all"]))


def test_packed_entry_points_check_their_arguments_without_launching():
    D.check_argument_codes(_lib().lib())
    torch.cuda.synchronize()


def test_wrappers_on_a_device_sampler_equal_filter():
    from esr_nerf_amd import regroup
    from esr_nerf_amd.config import AttrDict
    from esr_nerf_amd.data import RayGroupManager
    n_u, n_c = 5000, 333
    g = torch.Generator().manual_seed(2)
    perm = torch.randperm(n_u + n_c, generator=g)
    data = {k: torch.randn(n_u + n_c, 3, generator=g) for k in ("rays_o", "rays_d", "viewdirs")}
    cfg = AttrDict(system=dict(device="cuda:0", data_preload="cuda"))
    for name, f in _patterns(n_u, 5).items():
        flags = torch.from_numpy(f).to(DEV)
        words = regroup.pack_flags(flags)
        assert words.dtype == torch.int64 and np.array_equal(words.cpu().numpy().view(np.uint64), D.pack(f)), name
        back = regroup.unpack_flags(words, n_u)
        assert back.dtype == torch.bool and torch.equal(back, flags), name
        a, b = (RayGroupManager(cfg, data, list(data), 24, 8, 48, 16, perm[:n_u], perm[n_u:]) for _ in range(2))
        a.filter(flags)
        stats = regroup.new_stats(DEV)
        stats.copy_(regroup._identity())
        host = regroup.apply_flags(b, words, stats, packed=True)
        assert host["totals"] == (int(f.sum()), n_u - int(f.sum())), name
        assert torch.equal(a.uncert_data_idxs, b.uncert_data_idxs) and torch.equal(a.cert_data_idxs, b.cert_data_idxs), name
        assert b.uncert_data_idxs.is_cuda and b.uncert_data_idxs.is_contiguous() and b.cert_data_idxs.is_contiguous()
        assert (b.uncert_batch_st, b.cert_batch_st) == (48, 16)
    # decide_bits merges chunks that start on words into one record
    e = R.emission_case(5000, K, 3)
    ed = torch.from_numpy(e).to(DEV)
    _, st1 = regroup.decide(ed, K)
    words, st = torch.empty(D.n_words(5000), dtype=torch.int64, device=DEV), None
    for a in range(0, 5000, 1280):
        b = min(5000, a + 1280)
        _, st = regroup.decide_bits(ed[a:b], K, words[a // 64:D.n_words(b)], st)
    assert np.array_equal(words.cpu().numpy().view(np.uint64), D.pack(R.decide(e, np.float32(K))))
    assert not R.same_stats(regroup.read_stats(st), regroup.read_stats(st1))
    with pytest.raises(ValueError, match="packed flags"):
        regroup.decide_bits(ed, K, words[:-1])


@pytest.mark.parametrize("world,port", [(2, 29565), (3, 29567)])
def test_ranks_on_the_one_gpu_equal_the_single_process_byte_path(world, port):
    """Each rank a fresh child process under ``torch.distributed.run`` over gloo, all on the one GPU.  Stub renderer on the
    device (n = 5 * 64 + 37 with edge values and a NaN ray, n = 59, n = 0, a data_preload: cpu sampler, a camera-style set, a
    failing rank): index vectors, flags, statistics and counts equal those of the single-process byte path, exactly, on every
    rank.  The real g16 ``ESRNeRF`` model with ``k_val`` in the widest gap of the per-ray maxima between their quartiles (the
    worker asserts that the gap exceeds 1000 ulp of ``k_val``), array and camera-defined sets: flags and index vectors are
    exactly those of the single-process run on all ranks; then one ``LtsStep(stage="pdra", process_group=WORLD)`` step on
    ``sampler.sample()`` whose all-reduced loss is finite and the same on every rank."""
    out = run_ranks(["cuda:0", "stub,fail,model"], world, port, timeout=300)
    print(why(out))
    assert out.returncode == 0, why(out)
    assert all(f"DPREGROUP rank {r} of {world} ok" in out.stdout for r in range(world)), why(out)
