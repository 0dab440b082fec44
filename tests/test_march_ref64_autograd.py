"""The march restatement's backward (march_ref64.backward) against torch autograd in float64 through the CPU oracle's own
operations (oracle/fine_path.py: trilinear_explicit, sdf_stencil's clamped central differences, neus_alpha_interp /
neus_alpha_grad;
oracle/coarse_path.py's gradient-grid sampling), on small grids with the restatement's survivor set held fixed.  No GPU."""
from types import SimpleNamespace

import pytest
import torch

import feat_ref64 as FR
import march_ref64 as R
from oracle import fine_path as fp

F64 = torch.float64
REL = 1e-12


def _case(coarse, ga, seed):
    g = torch.Generator().manual_seed(seed)
    dims = (7, 9, 6)
    sc = R.box_scene(dims, vox=1.0 / 8, s_val=6.0, fast_thres=1e-4)
    N = 48
    ext = (sc.hi - sc.lo)
    o = sc.lo + ext * torch.rand(N, 3, generator=g) * 1.2 - 0.1 * ext
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=1)
    d[:6] = torch.tensor([0.0, 0.0, 1.0])                    # zero direction components
    o = o - d * 0.4
    zz = torch.linspace(-1, 1, dims[2])
    sdf = (zz[None, None, :] * 0.35 + 0.05 * torch.randn(*dims, generator=g)).float()
    mask = torch.full(dims, 5.0)
    mask[:, 2:4, :] = -8.0                                   # a pruned slab: gaps between survivors
    gg = (0.5 * torch.randn(*dims, 3, generator=g)).float() if (coarse and ga) else None
    inp = R.Inputs(rays_o=o.float(), rays_d=d.float(), viewdirs=torch.nn.functional.normalize(d, dim=1).float(),
                   mask=mask, sdf=sdf, gg=gg)
    return sc, inp


def _autograd(sc, inp, fw, gw, dlast):
    """Loss sum(gw * w) + sum(dlast * T_last) on the fixed survivor sets; gradient w.r.t. the SDF grid (and gg)."""
    live = fw.live
    ray = torch.nonzero(live)[:, 0]
    ind = fw.ind[live].double()
    size = torch.tensor(sc.dims, dtype=F64)
    norm = (ind / (size - 1) * 2 - 1).flip(-1)               # grid_sample order: component 0 addresses the last axis
    grid = inp.sdf.double()[None, None].clone().requires_grad_(True)
    s = fp.trilinear_explicit(grid, norm)[:, 0]
    ggrid = None
    if fw.ga:
        dist = torch.tensor(sc.stepdist, dtype=F64)
        if fw.coarse:
            ggrid = inp.gg.double().permute(3, 0, 1, 2)[None].clone().requires_grad_(True)
            grad = fp.trilinear_explicit(ggrid, norm)
        else:
            # sdf_stencil's radius-1 clamped central differences, at the kernel's binary32 tap indices (tap_index): a
            # float64 stencil would move each tap by ~1e-8 of a voxel
            case = SimpleNamespace(dims=sc.dims)
            cols = []
            for a in range(3):
                ixp, ap = FR.tap_index(case, fw.ind[live], a, 1.0)
                ixm, am = FR.tap_index(case, fw.ind[live], a, -1.0)
                tp = lambda ix: fp.trilinear_explicit(grid, (ix.double() / (size - 1) * 2 - 1).flip(-1))[:, 0]
                cols.append((tp(ixp) - tp(ixm)) / (ap - am).double() / sc.vox)
            grad = torch.stack(cols, -1)
        alpha = fp.neus_alpha_grad(inp.viewdirs.double(), ray, dist, s, grad, sc.s_val)
    else:
        alpha = fp.neus_alpha_interp(s, ray, sc.s_val)
    assert float((alpha.detach() - fw.alpha[live]).abs().max()) <= 1e-13
    A = torch.zeros(fw.s.shape, dtype=F64).index_put((ray, torch.nonzero(live)[:, 1]), alpha)
    om = torch.where(fw.proc, 1 - A, torch.ones_like(A))
    after = torch.cumprod(om, 1)
    before = torch.cat([torch.ones_like(after[:, :1]), after[:, :-1]], 1)
    w = torch.where(fw.proc, before * A, torch.zeros_like(A))
    loss = (torch.where(fw.v3, gw.double(), torch.zeros_like(A)) * w).sum() + (dlast.double() * after[:, -1]).sum()
    loss.backward()
    return grid.grad[0, 0].reshape(-1), None if ggrid is None else ggrid.grad[0].permute(1, 2, 3, 0).reshape(-1)


def _compare(cells, dense):
    u, v, _ = cells
    ref = torch.zeros_like(dense).index_add_(0, u, v)
    scale = float(dense.abs().max())
    assert scale > 0
    assert float((ref - dense).abs().max()) <= REL * scale, float((ref - dense).abs().max()) / scale


@pytest.mark.parametrize("coarse,ga", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_backward_equals_autograd(coarse, ga, seed):
    sc, inp = _case(coarse, ga, seed)
    fw = R.forward(sc, inp, coarse=coarse, ga=ga)
    assert int(fw.v3.sum()) > 10 and int((fw.proc & ~fw.v3).sum() + (fw.live & ~fw.proc).sum()) > 0
    g = torch.Generator().manual_seed(100 + seed)
    gw = torch.randn(fw.s.shape, generator=g, dtype=F64)
    dlast = torch.randn(fw.N, generator=g).float()
    bw = R.backward(sc, inp, fw, gw, dlast, eps=0.0)
    dsdf, dgg = _autograd(sc, inp, fw, gw, dlast)
    _compare(bw.grad_sdf, dsdf)
    if coarse and ga:
        _compare(bw.grad_gg, dgg)
    if not ga:                                               # the value-tap split: scattered + per-record == the whole
        bw2 = R.backward(sc, inp, fw, gw, dlast, rec_mode=True, eps=0.0)
        u, v, _ = bw2.grad_sdf
        part = torch.zeros_like(dsdf).index_add_(0, u, v)
        rr, vals, _ = bw2.dsdf
        r, j = torch.nonzero(fw.v3, as_tuple=True)
        fl, vv, _ = R._cells(fw.ind[r, j], vals, vals.abs(), sc.dims)
        keep = fl >= 0
        part.index_add_(0, fl[keep], vv[keep])
        assert float((part - dsdf).abs().max()) <= REL * float(dsdf.abs().max())
