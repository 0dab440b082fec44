"""CPU side of PDRA's ray re-split (esr_nerf_amd/regroup.py): the numpy restatement tests/regroup_ref.py against torch's
own statements and ``data.RayGroupManager.filter``, its edge cases, five mutants of it rejected, ``update_ray_groups`` with a
stub renderer against the reference's statements (app/fine/pdra.py:882-932), the refusals, and the C ABI's declarations."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import regroup_ref as R
from esr_nerf_amd import _lib, regroup
from esr_nerf_amd.config import AttrDict
from esr_nerf_amd.data import RayGroupManager

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("esr_emit_decide",)
K = 0.40575385
KEYS = ["rays_o", "rays_d", "viewdirs"]


def _cfg(preload="cpu"):
    return AttrDict(system=dict(device="cpu", data_preload=preload))


def _torch_decide(e, k):
    return (torch.max(torch.from_numpy(e), dim=-1)[0] > k).numpy()           # pdra.py:911


@pytest.mark.parametrize("n,seed", [(0, 0), (1, 1), (16, 2), (257, 3), (5000, 4)])
def test_restated_decision_and_statistics_equal_torch(n, seed):
    e = R.emission_case(n, K, seed)
    k32 = float(np.float32(K))
    f = R.decide(e, k32)
    assert f.dtype == np.bool_ and np.array_equal(f, _torch_decide(e, k32))
    s = R.stats(e, f)
    assert s["n_set"] + s["n_clear"] == n and s["n_set"] == int(f.sum())
    t = torch.from_numpy(e)
    assert s["n_nan"] == int(torch.isnan(t).any(1).sum())
    for tag, sel in (("all", np.ones(n, bool)), ("set", f), ("clear", ~f)):
        v = t[torch.from_numpy(sel)]
        v = v[~torch.isnan(v)]
        if v.numel():                                                        # equal as VALUES (torch leaves the zero's sign open)
            assert s[f"min_{tag}"] == float(v.min()) and s[f"max_{tag}"] == float(v.max()), tag
        else:
            assert s[f"min_{tag}"] == np.inf and s[f"max_{tag}"] == -np.inf, tag
    # the module's torch statements for CPU tensors agree as well
    f2, s2 = regroup._decide_torch(t, k32)
    assert np.array_equal(f2.numpy(), f) and all(s2[k] == s[k] for k in R.STAT_KEYS)


def test_edge_rays_are_decided_as_the_reference_decides_them():
    k = np.float32(K)
    rows = R.edge_rows(k)
    f = R.decide(rows, k)
    assert np.array_equal(f, _torch_decide(rows, float(k)))
    #          =k     =k,dn  up     dn     up     kkk    nan    nan+up nan    nan    inf   -inf   inf   zeros...
    assert f.tolist() == [False, False, True, False, True, False, False, False, False, False, True, False, True,
                          False, False, False]
    s = R.stats(rows, f)
    assert s["n_nan"] == 4 and s["n_set"] == 4 and s["n_clear"] == 12
    assert s["max_all"] == np.inf and s["min_all"] == -np.inf and s["min_set"] == -np.inf      # [lo, -inf, inf] is set
    # zeros around k_val = 0: -0.0 and +0.0 are both "not above 0"; the minimum of {-0.0, +0.0} is -0.0 by the total order
    z = np.array([[-0.0, 0.0, -0.0], [0.0, 0.0, 0.0]], np.float32)
    fz = R.decide(z, 0.0)
    assert not fz.any() and np.array_equal(fz, _torch_decide(z, 0.0))
    sz = R.stats(z, fz)
    assert np.signbit(sz["min_all"]) and not np.signbit(sz["max_all"])
    assert np.array_equal(R.order_key(np.float32([-np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf])),
                          np.sort(R.order_key(np.float32([-np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf]))))
    # empty, all set, all clear
    e0 = np.zeros((0, 3), np.float32)
    s0 = R.stats(e0, R.decide(e0, k))
    assert (s0["n_set"], s0["n_clear"], s0["n_nan"]) == (0, 0, 0) and s0["min_all"] == np.inf and s0["max_set"] == -np.inf
    e = R.emission_case(300, K, 9, edges=False)
    hi, lo = R.decide(e, -100.0), R.decide(e, 100.0)
    assert hi.all() and not lo.any()
    assert R.stats(e, hi)["min_clear"] == np.inf and R.stats(e, lo)["max_set"] == -np.inf
    assert R.stats(e, hi)["min_set"] == e.min() and R.stats(e, lo)["max_clear"] == e.max()


def _sampler(n_u, n_c, seed, preload="cpu", **kw):
    g = torch.Generator().manual_seed(seed)
    n = n_u + n_c
    perm = torch.randperm(n, generator=g)
    data = {"rays_o": torch.arange(n, dtype=torch.float32)[:, None].repeat(1, 3), "rays_d": torch.randn(n, 3, generator=g),
            "viewdirs": torch.randn(n, 3, generator=g)}
    return RayGroupManager(_cfg(preload), data, list(KEYS), 24, 8, uncert_data_idxs=perm[:n_u], cert_data_idxs=perm[n_u:], **kw)


@pytest.mark.parametrize("n_u,n_c,pattern", [(3000, 500, "random_1"), (3000, 500, "random_99"), (2500, 1, "runs"),
                                             (1025, 77, "alternating"), (40, 9, "all_set"), (40, 9, "all_clear")])
def test_restated_partition_equals_the_samplers_filter(n_u, n_c, pattern):
    s = _sampler(n_u, n_c, 3)
    u, c = s.uncert_data_idxs.numpy().copy(), s.cert_data_idxs.numpy().copy()
    f = R.flag_patterns(n_u, 7)[pattern]
    s.uncert_batch_st, s.cert_batch_st = 48, 16
    s.filter(torch.from_numpy(f))
    nu, nc = R.partition(u, c, f)
    assert np.array_equal(nu, s.uncert_data_idxs.numpy()) and np.array_equal(nc, s.cert_data_idxs.numpy())
    assert (s.uncert_batch_st, s.cert_batch_st) == (48, 16)
    # apply_flags on a CPU-home sampler is the same lines
    s2 = _sampler(n_u, n_c, 3)
    s2.uncert_batch_st, s2.cert_batch_st = 48, 16
    assert regroup.apply_flags(s2, torch.from_numpy(f)) is None
    assert torch.equal(s2.uncert_data_idxs, s.uncert_data_idxs) and torch.equal(s2.cert_data_idxs, s.cert_data_idxs)
    assert (s2.uncert_batch_st, s2.cert_batch_st) == (48, 16)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_each_mutant_of_the_restatement_is_rejected_on_a_small_case(mutant):
    k = np.float32(K)
    e = R.emission_case(64, k, 11)
    u, c = np.arange(100, 164)[::-1].copy(), np.arange(5)
    f = R.decide(e, k)
    assert 8 < f.sum() < 56
    good = R.partition(u, c, f)
    fm = R.decide(e, k, mutant)
    bad = R.partition(u, c, fm, mutant)
    if mutant in ("ge", "min_channel", "nan_uncertain"):
        assert not np.array_equal(fm, f), mutant
    assert not (np.array_equal(bad[0], good[0]) and np.array_equal(bad[1], good[1])), mutant
    # ... and the unmutated restatement is what torch says
    assert np.array_equal(f, _torch_decide(e, float(k)))
    tu, tc = torch.from_numpy(u), torch.from_numpy(c)
    assert np.array_equal(good[0], tu[torch.from_numpy(f)].numpy())
    assert np.array_equal(good[1], torch.cat([tc, tu[torch.from_numpy(~f)]]).numpy())


class StubRenderer:
    """``eval_emit`` hands back recorded rows: ``rays_o[:, 0]`` carries the original row of a ray"""

    def __init__(self, table, fail_at=None):
        self.table, self.fail_at = table, fail_at
        self.calls, self.modes_seen = [], []
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
        assert rays_o.shape == rays_d.shape == viewdirs.shape
        self.modes_seen.append(self.mode())
        if self.fail_at is not None and len(self.calls) == self.fail_at:
            raise RuntimeError("eval_emit failed")
        self.calls.append(len(rays_o))
        return self.table[rays_o[:, 0].long()]


def _reference_statements(stub, data, uncert, cert, k_val, bs):
    """pdra.py:887-927 and utils2/utils.py:264-267, 305-312 on plain tensors -> (uncert, cert, printed lines)"""
    line = lambda nu, nc: f"uncertain: {nu}\t certain: {nc}\t uncertain/all: {nu / (nu + nc) * 100}"
    out = ["[PREV]", line(len(uncert), len(cert)), f"curr k_val: {k_val}"]
    rays_o, rays_d, viewdirs = (data[k][uncert] for k in KEYS)
    emission = torch.zeros_like(rays_o)
    for idx in torch.arange(len(emission)).split(bs):
        emission[idx] = stub.eval_emit(rays_o=rays_o[idx], rays_d=rays_d[idx], viewdirs=viewdirs[idx])
    mask = torch.max(emission, dim=-1)[0] > k_val
    if emission.numel():
        out.append(f"emission(max, min): {float(emission.max())} {float(emission.min())}")
    if mask.sum():
        out.append(f"emission_uncert_masks(max, min): {float(emission[mask].max())} {float(emission[mask].min())}")
    if mask.bitwise_not().sum():
        out.append(f"emission_cert_masks(max, min): {float(emission[~mask].max())} {float(emission[~mask].min())}")
    cert = torch.cat([cert, uncert[~mask]])
    uncert = uncert[mask]
    out += ["[NEW MASK UPDATE]", line(len(uncert), len(cert))]
    return uncert, cert, out, mask, emission


@pytest.mark.parametrize("mode", ["train", "finetune", "eval"])
@pytest.mark.parametrize("bs", [4096, 500, None])
def test_update_ray_groups_with_a_stub_renderer_equals_the_references_statements(mode, bs, capsys):
    n_u, n_c = 9000, 700
    table = torch.from_numpy(R.emission_case(n_u + n_c, K, 21, edges=False))      # (the reference's prints take no NaN)
    s = _sampler(n_u, n_c, 4)
    assert s.home == "cpu" and not s.uncert_data_idxs.is_cuda
    s.uncert_batch_st, s.cert_batch_st = 72, 24
    u0, c0 = s.uncert_data_idxs.clone(), s.cert_data_idxs.clone()
    ref = StubRenderer(table)
    want_u, want_c, want_lines, want_mask, want_e = _reference_statements(ref, s.data, u0, c0, K, 4096)
    stub = StubRenderer(table)
    if mode != "train":
        stub.train(True, finetune=True) if mode == "finetune" else stub.eval()
    capsys.readouterr()
    rep = regroup.update_ray_groups(stub, s, K, batch_size=bs, return_emission=True)
    printed = capsys.readouterr().out.splitlines()
    assert stub.mode() == mode and set(stub.modes_seen) == {"eval"}
    size = regroup.DEFAULT_BATCH_SIZE if bs is None else bs
    assert stub.calls == [min(size, n_u - a) for a in range(0, n_u, size)]
    assert torch.equal(s.uncert_data_idxs, want_u) and torch.equal(s.cert_data_idxs, want_c)
    assert (s.uncert_batch_st, s.cert_batch_st) == (72, 24)
    assert printed == want_lines
    assert torch.equal(rep.flags, want_mask) and torch.equal(rep.emission, want_e)
    assert (rep.uncertain_before, rep.certain_before, rep.uncertain_after, rep.certain_after) == \
        (n_u, n_c, len(want_u), len(want_c))
    assert rep.k_val == K and not R.same_stats(rep.stats, R.stats(want_e.numpy(), want_mask.numpy()))
    assert 0 < len(want_u) < n_u
    # quiet, and without the emission
    s2 = _sampler(n_u, n_c, 4)
    rep2 = regroup.update_ray_groups(StubRenderer(table), s2, K, batch_size=bs, verbose=False)
    assert capsys.readouterr().out == "" and rep2.emission is None and torch.equal(rep2.flags, want_mask)


@pytest.mark.parametrize("mode", ["train", "finetune", "eval"])
def test_the_renderers_mode_is_restored_when_eval_emit_raises(mode):
    s = _sampler(1000, 10, 5)
    u0, c0 = s.uncert_data_idxs.clone(), s.cert_data_idxs.clone()
    stub = StubRenderer(torch.zeros(1010, 3), fail_at=1)
    if mode != "train":
        stub.train(True, finetune=True) if mode == "finetune" else stub.eval()
    with pytest.raises(RuntimeError, match="eval_emit failed"):
        regroup.update_ray_groups(stub, s, K, batch_size=300, verbose=False)
    assert stub.mode() == mode and stub.modes_seen == ["eval", "eval"]
    assert torch.equal(s.uncert_data_idxs, u0) and torch.equal(s.cert_data_idxs, c0)          # the groups are untouched


def test_empty_and_one_sided_groups():
    for n_u, k in ((0, K), (50, -100.0), (50, 100.0)):
        s = _sampler(n_u, 6, 6)
        u0, c0 = s.uncert_data_idxs.clone(), s.cert_data_idxs.clone()
        rep = regroup.update_ray_groups(StubRenderer(torch.rand(n_u + 6, 3)), s, k, verbose=False)
        keep = n_u if k < 0 else 0
        assert (rep.uncertain_after, rep.certain_after) == (keep, 6 + n_u - keep)
        assert torch.equal(s.uncert_data_idxs, u0[:keep]) and torch.equal(s.cert_data_idxs, torch.cat([c0, u0[keep:]]))


def test_misuse_is_refused_with_a_message():
    s = _sampler(100, 10, 7, rank=1, world=2)
    with pytest.raises(NotImplementedError, match="SAME flags"):
        regroup.update_ray_groups(StubRenderer(torch.zeros(110, 3)), s, K, verbose=False)
    assert "SAME flags" in regroup.__doc__
    # CPU tensors: there is no CPU kernel
    for call in (lambda: regroup.decide(torch.zeros(4, 3), K), lambda: regroup.partition(torch.arange(4), torch.ones(4, dtype=torch.bool))):
        with pytest.raises(RuntimeError, match="needs device tensors"):
            call()
    with pytest.raises(ValueError, match="flags for an uncertain group"):
        regroup.apply_flags(_sampler(10, 2, 8), torch.ones(9, dtype=torch.bool))
    with pytest.raises(ValueError, match="positive"):
        regroup.update_ray_groups(StubRenderer(torch.zeros(12, 3)), _sampler(10, 2, 8), K, batch_size=0)


def test_header_declares_the_regroup_entry_points_and_ctypes_agrees():
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    # the names only: tests/test_host.py checks every entry's restype and argument types against the header text
    for name in ENTRIES:
        assert name in _lib.EXPORTS and _lib.SIGNATURES[name][0] is ctypes.c_int, name
    assert int(re.search(r"#define ESR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    for name, val in (("ESR_PARTITION_BLOCK", _lib.PARTITION_BLOCK), ("ESR_PARTITION_SCAN_TILE", _lib.PARTITION_SCAN_TILE)):
        assert int(re.search(r"#define " + name + r" (\d+)", header).group(1)) == val
    assert _lib.PARTITION_BLOCK == R.TILE
    fields = [n for n, _ in _lib.EsrRegroupStats._fields_]
    assert tuple(fields) == R.STAT_KEYS == regroup.STAT_KEYS
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "esr_hip.h"\nint main(){printf("%zu",sizeof(esr_regroup_stats_t));\n'
           + "".join(f'printf(" %zu",offsetof(esr_regroup_stats_t,{n}));' for n in fields) + "return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes == [ctypes.sizeof(_lib.EsrRegroupStats)] + [getattr(_lib.EsrRegroupStats, n).offset for n in fields]
    assert sizes[0] == 48 and regroup._STATS_WORDS == 6


def test_entry_points_check_their_arguments_before_any_launch():
    """The argument checks run on the host: n == 0 succeeds without touching a pointer, a negative n is ESR_EINVAL, 2^31 rows
    are ESR_ECAP, a NULL pointer is ESR_EINVAL"""
    L = _lib.lib()
    null = ctypes.c_void_p(0)
    for n, code in ((0, 0), (-1, -1), (1 << 31, -2), ((1 << 31) + 5, -2), (5, -1)):
        assert L.esr_emit_decide(null, n, 0.5, null, null, 0, null) == code, n
        assert L.esr_emit_decide(null, n, 0.5, null, null, 1, null) == code, n
