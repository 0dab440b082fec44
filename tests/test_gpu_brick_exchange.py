"""The brick gradient exchange on the MI355X, bit for bit and past the launch cap: esr_brick_flags / _list / _pack / _unpack
through the C entry points against the numpy reference of brick_ref.py on its case tables (proved on the CPU by
test_brick_ref_host.py, where a list of planted defects fails them), and GridGradSync with the default HipBrickOps on two
real ranks against the bits of a0 + a1.  No comparison carries a tolerance.

Kernel level: every device buffer lies between two guard bands of 1 KiB that must come back bit-identical, inputs come
back bit-identical, outputs are pre-filled with the byte 0xA5 and keep it wherever the reference writes nothing.

Trips of the grid-stride loops (G = 32768 groups per trip, derived in brick_ref.py): buffers of G - 1 and G bricks take
one trip, G + 1 and G + 131 two, 2G + 3 three (3 bricks in the last one: the upper half of the last active wave is idle, as
at G + 1, G + 131 and 33 bricks); index lists of 1 and G slots take one trip, G + 1 two, 2G + 5 three.  In the two-rank run
scenario 9 has 2G + 3 bricks and a list of 2G + 1 slots: flags, pack and unpack take three trips each.

Two ranks (both on device 0, gloo), measured on the MI355X: the worker's loop over the thirteen steps of the scenario table
takes 0.5 s, the whole test with the start of the two processes 4.8 s; the 146 kernel-level cases take 2 s together."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import brick_ref as R
from conftest import ROOT
from test_gpu_dp import _why

pytestmark = pytest.mark.gpu

DEV = "cuda"
GB = 1024                       # bytes of guard in front of and behind every buffer (keeps the payload 16-byte aligned)
EINVAL = -1                     # ESR_EINVAL (include/esr_hip.h)
NULL = C.c_void_p(0)


def _L():
    from esr_nerf_amd import _lib
    return _lib.lib(), _lib.stream_ptr(DEV)


class Band:
    """a device buffer holding `payload`'s bytes between two guard bands of PAT"""
    def __init__(self, payload):
        raw = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        host = np.full(GB + raw.size + GB, R.PAT, np.uint8)
        host[GB:GB + raw.size] = raw
        self.init, self.nbytes = raw.copy(), raw.size
        self.buf = torch.from_numpy(host).to(DEV)

    def ptr(self, byte_off=0):
        return C.c_void_p(self.buf.data_ptr() + GB + byte_off)

    def read(self, dtype=np.uint8):
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        assert (host[:GB] == R.PAT).all(), "the guard in front of a buffer was written"
        assert (host[GB + self.nbytes:] == R.PAT).all(), "the guard behind a buffer was written"
        return host[GB:GB + self.nbytes].view(dtype).copy()

    def unchanged(self):
        return bool(np.array_equal(self.read(), self.init))


def pat(n, dtype):
    return np.full(n * np.dtype(dtype).itemsize, R.PAT, np.uint8).view(dtype)


class Hip:
    """brick_ref.run_case's `impl` on the C entry points of csrc/brick.hip"""
    def __init__(self):
        self.L, self.s = _L()
        self.scratch = Band(np.full(int(self.L.esr_brick_list_scratch_ints()), 0x5A5A5A5A, np.int32))

    def flags(self, x):
        bx, bf = Band(x), Band(pat(R.n_bricks(x.size), np.uint8))
        assert self.L.esr_brick_flags(bx.ptr(), C.c_int64(x.size), bf.ptr(), self.s) == 0
        out = bf.read()
        assert bx.unchanged()
        return out

    def pack(self, x, idx):
        bx, bi, bp = Band(x), Band(idx), Band(pat(idx.size * R.BRICK, np.float32))
        assert self.L.esr_brick_pack(bx.ptr(), C.c_int64(x.size), bi.ptr(), C.c_int64(idx.size), bp.ptr(), self.s) == 0
        out = bp.read(np.float32)
        assert bx.unchanged() and bi.unchanged()
        return out

    def unpack(self, packed, idx, x):
        bx, bi, bp = Band(x), Band(idx), Band(packed)
        assert self.L.esr_brick_unpack(bp.ptr(), bi.ptr(), C.c_int64(idx.size), bx.ptr(), C.c_int64(x.size), self.s) == 0
        out = bx.read(np.float32)                       # (read() checks the guard behind the buffer)
        assert bp.unchanged() and bi.unchanged()
        return out, None

    def list(self, flags, cap, scratch):
        bf, bi, bc = Band(flags), Band(pat(cap, np.int64)), Band(pat(1, np.int64))
        rc = self.L.esr_brick_list(bf.ptr() if flags.size else NULL, C.c_int64(flags.size), C.c_int64(cap),
                                   bi.ptr() if cap else NULL, bc.ptr(), self.scratch.ptr(), self.s)
        assert rc == 0
        idx, count = bi.read(np.int64), bc.read(np.int64)
        self.scratch.read()
        assert bf.unchanged()
        return idx, int(count[0])


@pytest.fixture(scope="module")
def hip():
    return Hip()


@pytest.mark.parametrize("case", R.cases())
def test_hip_kernel_gives_the_reference_bits(hip, case):
    why = R.run_case(hip, case)
    assert why is None, (case, why)


def test_list_of_no_bricks(hip):
    idx, count = hip.list(np.zeros(0, np.uint8), 3, None)
    assert count == 0 and (idx == -1).all()


def test_return_codes_and_nothing_written(hip):
    """0 for n == 0 and n_idx == 0, ESR_EINVAL for negative sizes, NULL pointers and a `buf` or `packed` that is not 16-byte
    aligned (a view offset by one float); nothing is written in any of these calls."""
    L, s = hip.L, hip.s
    x = R.buffer("nb33_t3")
    idx = R.index_lists("nb33_t3")["asc_neg"][0]
    n, k = C.c_int64(x.size - 1), C.c_int64(idx.size - 1)               # (a view offset by one float is one float shorter)
    bx, bi = Band(x), Band(idx)
    bf, bp = Band(pat(R.n_bricks(x.size), np.uint8)), Band(pat(idx.size * R.BRICK, np.float32))
    bl, bc = Band(pat(8, np.int64)), Band(pat(1, np.int64))
    zero, neg = C.c_int64(0), C.c_int64(-1)
    calls = [
        (0, L.esr_brick_flags, (bx.ptr(), zero, bf.ptr(), s)),
        (0, L.esr_brick_flags, (NULL, zero, NULL, s)),
        (EINVAL, L.esr_brick_flags, (bx.ptr(), neg, bf.ptr(), s)),
        (EINVAL, L.esr_brick_flags, (NULL, n, bf.ptr(), s)),
        (EINVAL, L.esr_brick_flags, (bx.ptr(), n, NULL, s)),
        (EINVAL, L.esr_brick_flags, (bx.ptr(4), n, bf.ptr(), s)),
        (0, L.esr_brick_pack, (bx.ptr(), n, bi.ptr(), zero, bp.ptr(), s)),
        (EINVAL, L.esr_brick_pack, (bx.ptr(), neg, bi.ptr(), k, bp.ptr(), s)),
        (EINVAL, L.esr_brick_pack, (bx.ptr(), n, bi.ptr(), neg, bp.ptr(), s)),
        (EINVAL, L.esr_brick_pack, (NULL, n, bi.ptr(), k, bp.ptr(), s)),
        (EINVAL, L.esr_brick_pack, (bx.ptr(), n, NULL, k, bp.ptr(), s)),
        (EINVAL, L.esr_brick_pack, (bx.ptr(), n, bi.ptr(), k, NULL, s)),
        (EINVAL, L.esr_brick_pack, (bx.ptr(4), n, bi.ptr(), k, bp.ptr(), s)),
        (EINVAL, L.esr_brick_pack, (bx.ptr(), n, bi.ptr(), k, bp.ptr(4), s)),
        (0, L.esr_brick_unpack, (bp.ptr(), bi.ptr(), zero, bx.ptr(), n, s)),
        (EINVAL, L.esr_brick_unpack, (bp.ptr(), bi.ptr(), k, bx.ptr(), neg, s)),
        (EINVAL, L.esr_brick_unpack, (bp.ptr(), bi.ptr(), neg, bx.ptr(), n, s)),
        (EINVAL, L.esr_brick_unpack, (NULL, bi.ptr(), k, bx.ptr(), n, s)),
        (EINVAL, L.esr_brick_unpack, (bp.ptr(), NULL, k, bx.ptr(), n, s)),
        (EINVAL, L.esr_brick_unpack, (bp.ptr(), bi.ptr(), k, NULL, n, s)),
        (EINVAL, L.esr_brick_unpack, (bp.ptr(4), bi.ptr(), k, bx.ptr(), n, s)),
        (EINVAL, L.esr_brick_unpack, (bp.ptr(), bi.ptr(), k, bx.ptr(4), n, s)),
        (EINVAL, L.esr_brick_list, (bf.ptr(), neg, C.c_int64(8), bl.ptr(), bc.ptr(), hip.scratch.ptr(), s)),
        (EINVAL, L.esr_brick_list, (bf.ptr(), C.c_int64(33), neg, bl.ptr(), bc.ptr(), hip.scratch.ptr(), s)),
        (EINVAL, L.esr_brick_list, (NULL, C.c_int64(33), C.c_int64(8), bl.ptr(), bc.ptr(), hip.scratch.ptr(), s)),
        (EINVAL, L.esr_brick_list, (bf.ptr(), C.c_int64(33), C.c_int64(8), NULL, bc.ptr(), hip.scratch.ptr(), s)),
        (EINVAL, L.esr_brick_list, (bf.ptr(), C.c_int64(33), C.c_int64(8), bl.ptr(), NULL, hip.scratch.ptr(), s)),
        (EINVAL, L.esr_brick_list, (bf.ptr(), C.c_int64(33), C.c_int64(8), bl.ptr(), bc.ptr(), NULL, s)),
    ]
    before = hip.scratch.read()
    for i, (want, fn, args) in enumerate(calls):
        assert fn(*args) == want, (i, fn.__name__, want)
    for b in (bx, bi, bf, bp, bl, bc):
        assert b.unchanged()
    assert np.array_equal(hip.scratch.read(), before)


def test_two_real_ranks_get_the_bits_of_a0_plus_a1():
    """brick_ref's scenario table (disjoint, overlapping, one rank all zero, a0 == -a1, the same again with trailing -1 slots,
    overflow completed by verify(), a union shrunk to a tenth, the dense branch, 2G + 3 bricks with a list of 2G + 1 slots,
    n < 128) on two processes sharing the GPU over gloo, each with product GridGradSync objects on the default
    HipBrickOps: after reduce() and verify() every rank holds the int32 bits of a0 + a1, and `last` is what the table says."""
    with tempfile.TemporaryDirectory() as d:
        w = os.path.join(d, "w.py")
        open(w, "w").write(R.WORKER)
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
        out = subprocess.run(
            [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
             "--master-addr", "127.0.0.1", "--master-port", "29573", w, ROOT, "cuda"],
            env=env, capture_output=True, text=True, timeout=300)
    lines = [l for l in out.stdout.splitlines() if l.startswith("BRICKX")]
    print("\n".join(lines))
    assert out.returncode == 0, _why(out)
    assert len(lines) == len(R.scenarios()) + 1 and lines[-1].startswith("BRICKX done")
