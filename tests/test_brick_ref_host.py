"""The case tables of the brick gradient exchange (tests/brick_ref.py) proved on the CPU, before a GPU sees them:
the numpy emulation of csrc/brick.hip's decomposition passes every case bit for bit against the reference, the torch
double (tests/brick_ops_double.py) passes the cases it supports (flags, pack, unpack), every planted defect (MUTANTS) is
rejected by a case that the test names, and the two-rank scenario table gives the expected bits and takes the expected
branches over gloo on CPU tensors with the torch double."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import brick_ref as R
from brick_ops_double import TorchBrickOps
from conftest import ROOT


def test_groups_per_trip_follow_from_the_launch_lines():
    """G = 32768 is derived from the launch lines of csrc/brick.hip (brick_ref's docstring): a changed block size, cap or brick
    size fails here instead of silently moving the sizes off the trip boundaries."""
    src = open(os.path.join(ROOT, "esr_nerf_amd", "csrc", "brick.hip")).read()
    common = open(os.path.join(ROOT, "esr_nerf_amd", "csrc", "esr_common.h")).read()
    launches = re.findall(r"esr_grid_for\((\w+) \* (\d+), (\d+), (\d+) \* (\d+)\), (\d+),", src)
    assert len(launches) == 3 and len(re.findall(r"esr_grid_for\(", src)) == 3
    for what, lanes, block, c0, c1, threads in launches:
        assert what in ("nb", "n_idx")
        assert (int(lanes), int(block), int(c0) * int(c1), int(threads)) == (R.GROUP, R.BLOCK, R.GRID_CAP, R.BLOCK)
    assert "int64_t g = (n + block - 1) / block;" in common and "if (g > cap) g = cap;" in common
    assert re.search(r"constexpr int BRICK = (\d+);", src).group(1) == str(R.BRICK)
    assert re.search(r"constexpr int LIST_BLOCKS = (\d+), LIST_THREADS = (\d+);", src).groups() == (str(R.LIST_BLOCKS), str(R.LIST_THREADS))
    assert R.G == R.GRID_CAP * R.BLOCK // R.GROUP == 32768
    assert R._launch_groups(33) == 40 and R._launch_groups(R.G + 1) == R.G and R._launch_groups(1) == 8


def test_case_tables_cover_what_they_claim():
    sizes = {nb for nb, n, t in R.BUFFERS.values()}
    G = R.G
    assert sizes >= {1, 31, 32, 33, G - 1, G, G + 1, 2 * G + 3}
    for nb in (G - 1, G, G + 1, 2 * G + 3):
        assert sum(1 for b, n, t in R.BUFFERS.values() if b == nb and n == nb * 128) == 1
    assert {n % 128 for nb, n, t in R.BUFFERS.values() if nb == 2 * G + 3} >= {0, 1, 3, 4, 5, 127}
    assert any((nb % R._launch_groups(nb)) % 2 == 1 for nb, n, t in R.BUFFERS.values())      # a half-idle last wave
    x = R.buffer("2G+3_t5")
    bits = R.u32(x)
    assert bits[-1] != 0 and not bits[-5:-1].any()                       # the ragged brick: only its very last element
    spec, blocks = R.special_bricks(*R.BUFFERS["2G+3_t5"][:2])
    assert blocks[0][0] + blocks[0][1] <= G and blocks[1][0] + blocks[1][1] > 2 * G            # first trip, last trip
    assert R.special_bricks(*R.BUFFERS["G+131"][:2])[1][1][0] >= G                             # a block wholly in the last trip
    f = R.flags_ref(x)
    for b, (name, pattern, flagged) in spec.items():
        row = bits[b * 128:(b + 1) * 128]
        assert (row != 0).sum() == 1 and pattern in row and f[b] == flagged, (b, name)
    for first, cnt in blocks:
        blk = bits[first * 128:(first + cnt) * 128].reshape(cnt, 128)
        assert ((blk != 0) == np.eye(cnt, dtype=bool)).all()
    assert (f == 0).sum() > f.size // 2                                  # all-zero bricks in between
    lists = R.index_lists("2G+3_t5")
    assert {a.size for a, _ in lists.values()} >= {1, G, G + 1, 2 * G + 5}
    last = 2 * G + 2
    a, p = lists["asc_2G5_neg"][0], lists["perm_2G5_neg"][0]
    assert int(np.flatnonzero(a == last)[0]) >= 2 * G and int(np.flatnonzero(p == last)[0]) < G
    assert (a[-3:] == -1).all() and (a[:G] == -1).any() and (np.diff(a[a >= 0]) > 0).all() and not (np.diff(p[p >= 0]) > 0).all()
    assert (lists["all_neg"][0] == -1).all()
    for name, (idx, for_unpack) in lists.items():
        real = idx[idx >= 0]
        assert idx.min() >= -1 and idx.max(initial=-1) <= last
        assert (np.unique(real).size == real.size) == for_unpack, name
    for nb in R.LIST_NB:
        assert set(np.unique(R.list_flags(nb, "0.3"))) <= {0, 1, 2, 255}
    assert set(np.unique(R.list_flags(65537, "0.3"))) == {0, 1, 2, 255}


class Torch:
    """run_case's `impl` on the torch double; outputs are pre-filled with PAT like the emulation's"""
    ops = TorchBrickOps()

    def flags(self, x):
        out = torch.full((R.n_bricks(x.size),), R.PAT, dtype=torch.uint8)
        self.ops.flags(torch.from_numpy(x.copy()), out)
        return out.numpy()

    def pack(self, x, idx):
        out = torch.from_numpy(np.full(idx.size * 128, R.PAT32, np.uint32).view(np.float32).copy())
        self.ops.pack(torch.from_numpy(x.copy()), torch.from_numpy(idx.copy()), out)
        return out.numpy()

    def unpack(self, packed, idx, x):
        flat = torch.from_numpy(x.copy())
        self.ops.unpack(torch.from_numpy(packed.copy()), torch.from_numpy(idx.copy()), flat)
        return flat.numpy(), None


def test_emulation_and_torch_double_give_the_reference_bits_on_every_case():
    emu, double, scratch = R.Emu(), Torch(), R.Scratch()
    n = 0
    for case in R.cases():
        why = R.run_case(emu, case, scratch)
        assert why is None, ("emulation", case, why)
        if not case.startswith("list"):
            why = R.run_case(double, case)
            assert why is None, ("torch double", case, why)
        n += 1
    assert n == len(R.cases()) and n > 100


@pytest.mark.parametrize("mut", sorted(R.MUTANTS))
def test_every_mutant_is_rejected_by_a_named_case(mut, capsys):
    """every operation a planted defect changes fails a case; which one is printed (also without -s)"""
    impl, scratch = R.Emu(mut), R.Scratch()
    kinds, what = R.MUTANTS[mut]
    caught = {}
    for case in R.cases():
        kind = case.split("/")[0].rstrip("2")
        if kind not in kinds or kind in caught:
            continue
        why = R.run_case(impl, case, scratch)
        if why is not None:
            caught[kind] = (case, why)
    with capsys.disabled():
        print("\nmutant %-18s (%s)" % (mut, what))
        for kind in kinds:
            print("    rejected by %-28s %s" % (caught.get(kind, ("NOTHING", ""))))
    assert set(caught) == set(kinds), (mut, "not rejected in", set(kinds) - set(caught))


def test_two_rank_scenarios_on_gloo_with_the_torch_double(capsys):
    """the scenario table of the GPU test (brick_ref.run_two_rank) on two gloo ranks with CPU tensors and the torch double: the
    expected bits of a0 + a1 after reduce() and verify(), and the expected mode / union / bricks / sent / overflow of every step."""
    names = [s["name"] for s in R.scenarios()]
    assert [n.split()[0] for n in names] == ["1", "2", "3", "4", "5", "6", "7", "8", "8", "9", "9", "10", "10"]
    by = {s["name"]: s for s in R.scenarios()}
    assert not np.intersect1d(*by["1 disjoint"]["sets"]).size and np.intersect1d(*by["2 overlapping"]["sets"]).size
    assert by["6 grows"]["union"] > 1.25 * by["5 the same again"]["union"] and by["6 grows"]["overflow"] > 0
    assert by["7 shrinks"]["union"] <= by["6 grows"]["union"] // 10
    s9 = by["9 2G+3 bricks, three trips"]
    assert s9["bricks"] == 2 * R.G + 3 and s9["n"] % 128 and 0.15 < s9["union"] / s9["bricks"] < 0.25 and s9["sent"] > 2 * R.G
    assert by["10 n < 128"]["n"] < 128
    s4 = by["4 a0 == -a1"]
    a0, a1 = R.rank_buffer(s4, 0), R.rank_buffer(s4, 1)
    c = s4["cancel"][0]
    assert (a0[c * 128:(c + 1) * 128] != 0).any() and not R.u32(a0[c * 128:(c + 1) * 128] + a1[c * 128:(c + 1) * 128]).any()
    with tempfile.TemporaryDirectory() as d:
        w = os.path.join(d, "w.py")
        open(w, "w").write(R.WORKER)
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
        out = subprocess.run(
            [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
             "--master-addr", "127.0.0.1", "--master-port", "29571", w, ROOT, "cpu"],
            env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("BRICKX")]
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert len(lines) == len(names) + 1 and lines[-1].startswith("BRICKX done")
