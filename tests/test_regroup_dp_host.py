"""CPU side of PDRA's re-split under data parallelism (esr_nerf_amd/regroup.py over csrc/regroup.hip): the ranks' shares,
the packed flag words against numpy, ``apply_flags`` on words, ``update_ray_groups(..., process_group=)`` with two and three real
gloo ranks and a stub renderer against the single-process run (tests/regroup_dp_ref.py: WORKER), and the C ABI's declarations."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import regroup_dp_ref as D
import regroup_ref as R
from esr_nerf_amd import _lib, regroup
from esr_nerf_amd.config import AttrDict
from esr_nerf_amd.data import RayGroupManager

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("esr_emit_decide_bits", "esr_flags_pack", "esr_flags_unpack", "esr_flag_scan_bits", "esr_index_partition_bits",
           "esr_regroup_stats_merge")


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128, 1000])
def test_shares_are_disjoint_ordered_whole_words_and_cover_the_group(n, world):
    shares = [regroup.ray_share(n, r, world) for r in range(world)]
    assert shares == [D.ray_share(n, r, world) for r in range(world)]
    assert shares[0][0] == 0 and shares[-1][1] == n
    for (lo, hi), (lo2, _) in zip(shares[:-1], shares[1:]):
        assert hi == lo2                                             # ordered, disjoint, no gap
    sizes = [hi - lo for lo, hi in shares]
    assert all(lo % 64 == 0 and 0 <= lo <= hi <= n for lo, hi in shares)
    assert max(sizes) - min(sizes) <= 64 and sum(sizes) == n
    if D.n_words(n) < world:
        assert sizes.count(0) == world - D.n_words(n)                # W < world: some ranks own no word
    with pytest.raises(ValueError):
        regroup.ray_share(n, world, world)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128, 1000, 4133])
def test_restated_packing_equals_numpys_little_endian_packbits_and_inverts(n):
    for name, f in R.flag_patterns(n, n + 3).items():
        words = D.pack(f)
        assert words.dtype == np.uint64 and len(words) == D.n_words(n)
        by_numpy = np.packbits(f, bitorder="little")
        want = np.zeros(8 * len(words), np.uint8)
        want[:len(by_numpy)] = by_numpy
        assert words.astype("<u8").tobytes() == want.tobytes(), name  # (bit 0 = the least significant bit of byte 0)
        assert np.array_equal(D.unpack(words, n), f), name
        if n % 64:
            assert int(words[-1]) >> (n % 64) == 0, name                # the tail of the last word is clear
        # the module's statements for CPU tensors are the same words; any non-zero byte is a set flag
        u8 = f.astype(np.uint8) * 255
        for given in (torch.from_numpy(f), torch.from_numpy(u8)):
            got = regroup.pack_flags(given)
            assert got.dtype == torch.int64 and np.array_equal(got.numpy().view(np.uint64), words), name
        back = regroup.unpack_flags(torch.from_numpy(words.view(np.int64)), n)
        assert back.dtype == torch.bool and np.array_equal(back.numpy(), f), name
        assert set(np.unique(back.view(torch.uint8).numpy())) <= {0, 1}


def _sampler(n_u, n_c, seed):
    g = torch.Generator().manual_seed(seed)
    n = n_u + n_c
    perm = torch.randperm(n, generator=g)
    data = {k: torch.randn(n, 3, generator=g) for k in ("rays_o", "rays_d", "viewdirs")}
    return RayGroupManager(AttrDict(system=dict(device="cpu", data_preload="cpu")), data, list(data), 24, 8, 48, 16,
                           uncert_data_idxs=perm[:n_u], cert_data_idxs=perm[n_u:])


def test_apply_flags_takes_packed_words_by_keyword_only():
    n_u = 1000
    for name, f in R.flag_patterns(n_u, 5).items():
        a, b = _sampler(n_u, 30, 3), _sampler(n_u, 30, 3)
        a.filter(torch.from_numpy(f))
        words = regroup.pack_flags(torch.from_numpy(f))
        assert regroup.apply_flags(b, words, packed=True) is None
        assert torch.equal(a.uncert_data_idxs, b.uncert_data_idxs) and torch.equal(a.cert_data_idxs, b.cert_data_idxs), name
        assert (b.uncert_batch_st, b.cert_batch_st) == (48, 16)
    # an int64 vector is never taken for words by its dtype, and words of the wrong length are refused
    s = _sampler(64, 3, 1)
    with pytest.raises(ValueError):
        regroup.apply_flags(s, torch.ones(64, dtype=torch.int64))
    with pytest.raises(ValueError, match="packed flags"):
        regroup.apply_flags(s, torch.ones(2, dtype=torch.int64), packed=True)
    with pytest.raises(ValueError, match="packed flags"):
        regroup.apply_flags(s, torch.ones(64, dtype=torch.bool), packed=True)
    with pytest.raises(TypeError):
        regroup.apply_flags(s, torch.ones(1, dtype=torch.int64), None, True)


def test_merged_records_of_the_restatement_equal_the_record_of_the_whole():
    k = np.float32(0.40575385)
    e = R.emission_case(900, k, 17)
    f = R.decide(e, k)
    whole = R.stats(e, f)
    for cuts in ((0, 900), (0, 300, 900), (0, 1, 64, 64, 500, 900)):
        parts = [R.stats(e[a:b], f[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        assert not R.same_stats(D.merge_records(parts), whole), cuts


def run_ranks(worker_args, world, port, timeout):
    """The worker of tests/regroup_dp_ref.py under torch.distributed.run -> the finished process"""
    with tempfile.TemporaryDirectory() as d:
        w = os.path.join(d, "w.py")
        with open(w, "w") as f:
            f.write(D.WORKER)
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
        return subprocess.run(
            [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
             "--master-addr", "127.0.0.1", "--master-port", str(port), w, ROOT, *worker_args],
            env=env, capture_output=True, text=True, timeout=timeout)


def why(out):
    keep = [l for l in (out.stdout + "\n" + out.stderr).splitlines()
            if any(k in l for k in ("Error", "error", "assert", "Traceback", "File \"", "DPREGROUP", "DPMODEL", "exitcode"))
            and "elastic/errors" not in l]
    return "\n".join(keep[-40:])


@pytest.mark.parametrize("world,port", [(2, 29561), (3, 29563)])
def test_gloo_ranks_with_a_stub_renderer_equal_the_single_process_run(world, port):
    """Every rank's index vectors, batch starts, report counts, statistics and flags equal those of a single-process run on
    a world = 1 copy of the sampler, exactly; each rank called eval_emit with the rows of its own share only; edge values,
    a NaN ray, n = 59 (rank 0's share is empty), n = 0, a data_preload: cpu sampler and a camera-style sampler; then a stub
    that raises on rank 1 only: every rank raises, with its renderer's mode back and its groups untouched.  (On the parent
    commit ``process_group=`` is an unknown keyword.)"""
    out = run_ranks(["cpu", "stub,fail"], world, port, timeout=240)
    assert out.returncode == 0, why(out)
    assert all(f"DPREGROUP rank {r} of {world} ok" in out.stdout for r in range(world)), why(out)


def test_a_sampler_of_many_ranks_is_still_refused_without_a_process_group():
    s = _sampler(100, 10, 7)
    s.rank, s.world = 1, 2
    with pytest.raises(NotImplementedError, match="SAME flags"):
        regroup.update_ray_groups(None, s, 0.5, verbose=False)
    assert "SAME flags" in regroup.__doc__ and "all_reduce(SUM)" in regroup.__doc__


def test_header_declares_the_packed_entry_points_and_ctypes_agrees():
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    # the names only: tests/test_host.py checks every entry's restype and argument types against the header text
    for name in ENTRIES:
        assert name in _lib.EXPORTS and _lib.SIGNATURES[name][0] is ctypes.c_int and hasattr(_lib.lib(), name), name
    assert int(re.search(r"#define ESR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == _lib.lib().esr_abi_version()
    assert _lib.PARTITION_BLOCK % 64 == 0 and _lib.PARTITION_BLOCK // 64 == 16


def test_packed_entry_points_check_their_arguments_before_any_launch():
    D.check_argument_codes(_lib.lib())
