"""The fine-feature check without a GPU: feat_check's flows (the comparison tests/test_gpu_feat_scatter.py runs on the kernels)
on the binary32 emulation feat_emu.Emu -- inside the bound of feat_ref64.K_FAMILY on the GPU test's own `tiny` and `odd`
cases (the bound is not too tight, the inputs are admissible) --, on every mutant of feat_emu.MUTANTS -- a miss in each
family the mutant lists, on at least one host case (the bound has teeth) --, the census the GPU test requires, the agreement
of feat_ref64.census with the emulation's own bookkeeping, the bar reach property of the forward, and the checker on a
backend with four planted errors."""
import math

import pytest
import torch

import feat_check as F
import feat_emu as E
import feat_ref64 as R


class HostEmu(E.Emu):
    """The emulation, plus after every backward: feat_ref64.census against the emulation's own segments and has flags."""

    def __init__(self, case, mut=None, nwaves=2048):
        super().__init__(case, mut, nwaves)
        self.disagree = []

    def bwd(self, X, gn):
        out = super().bwd(X, gn)
        tb, _ = self.case.launch_range()
        tiles, _ = R.census(self.case)
        seen = set()
        for n, info in enumerate(tiles):
            t = tb + n
            mine = self.book.get(t)
            if info is None:
                if mine is not None:
                    self.disagree.append(f"tile {t}: segments in the emulation, none in the census")
                continue
            seen.add(t)
            if mine is None:
                self.disagree.append(f"tile {t}: in the census, not in the emulation's launch")
                continue
            got = (mine["segs"], mine["cut8"], {k: mine["has"][k] for k in info["has"]})
            if got != (info["segs"], info["cut8"], info["has"]):
                self.disagree.append(f"tile {t}: emulation {got} != census {(info['segs'], info['cut8'], info['has'])}")
        return out


def _maker(mut, log, **kw):
    def make(case):
        e = HostEmu(case, mut, **kw)
        log.append(e)
        return e
    return make


def _small_uncovered(make, ck):
    """flow_uncovered's situation on a launch of 4 waves: tiles 4..7 are uncovered tiles that follow covered ones."""
    g = torch.Generator().manual_seed(650)
    case = F._base_case(F.GRIDS["tiny"], 1, seed=6)
    ro, rd, rr, rs, tiles = F.ray_records(case, [("axis", 8)], g)
    T = 8
    assert tiles >= T
    case.rays_o, case.rays_d, case.rec_ray, case.rec_step, case.tiles_all = ro, rd, rr[:T * 32], rs[:T * 32], T
    case.rec_sdf = torch.randn(T * 32, generator=g)
    case.srcs = [R.Src(F._dX(T, g) * 10, 0, 4, on=True, off=True)]
    case.dsdf_extra = torch.randn(T * 32, generator=g)
    F.run("uncovered/4 waves", case, make(case), dict(), ck)


def _gaps(make, ck):
    """Host-only: one ray's samples on both sides of a padding lane (a new segment must start after the gap), ray 0 right
    after a padding lane, and a diagonal ray cut into runs of 8 that starts mid-tile (cut8 counts from the segment's start)."""
    g = torch.Generator().manual_seed(660)
    case = F._base_case(F.GRIDS["tiny"], 1, seed=6)
    lo, hi = case.lo, case.hi
    c = (lo + hi) / 2
    d = torch.tensor([1.0, 1.0, 0.3])
    case.rays_o = torch.stack([c - d * 0.2, c - d * 0.2 + torch.tensor([0.05, -0.1, 0.0])]).float()
    case.rays_d = torch.stack([d, d]).float()
    rr = [-1] + [0] * 5 + [-1] + [0] * 5 + [-1, -1] + [1] * 18
    rs = [0] + list(range(20, 25)) + [0] + list(range(40, 45)) + [0, 0] + list(range(10, 46, 2))
    rr2 = [1] * 3 + [0] * 29
    rs2 = [4, 5, 6] + list(range(3, 61, 2))
    case.rec_ray = torch.tensor(rr + rr2, dtype=torch.int32)
    case.rec_step = torch.tensor(rs + rs2, dtype=torch.int32)
    case.tiles_all = 2
    p, valid = R.positions(case)
    assert bool(F._inside(case, p[valid]).all())
    case.rec_sdf = torch.randn(64, generator=g)
    case.srcs = [R.Src(F._dX(2, g), 0, 2, on=True, off=True)]
    F.run("gaps", case, make(case), dict(cut8_global=1, mixed=1), ck)


# host cases, cheapest first: name -> flow(make, ck)
HOST_CASES = {
    "one tile": F.flow_one_tile,
    "gaps": _gaps,
    "uncovered/4 waves": _small_uncovered,
    "tiny/groups": lambda mk, ck: F.flow_groups("tiny", mk, ck),
    "tiny/flat": lambda mk, ck: F.flow_flat("tiny", mk, ck),
    "tiny/faces": lambda mk, ck: F.flow_faces("tiny", mk, ck),
    "odd/groups": lambda mk, ck: F.flow_groups("odd", mk, ck),
    "odd/flat": lambda mk, ck: F.flow_flat("odd", mk, ck),
    "odd/faces": lambda mk, ck: F.flow_faces("odd", mk, ck),
    **{f"abi/{x}": (lambda mk, ck, x=x: F.flow_partial_sources(x, mk, ck)) for x in F.PARTIAL_EXTRAS},
    "abi/sources": F.flow_multi_source,
    # a 40^3 twin of the g256 runs, reaching the last cell
    "prod40": lambda mk, ck: F.flow_production(mk, ck, dims=(40, 40, 40), need=dict(fit=30, clip_hi=1), tag="prod40"),
    "tiny/points": lambda mk, ck: F.flow_explicit_points("tiny", mk, ck),
    "odd/points": lambda mk, ck: F.flow_explicit_points("odd", mk, ck),
    "tiny/rays": lambda mk, ck: F.flow_record_mode("tiny", mk, ck),
    "odd/rays": lambda mk, ck: F.flow_record_mode("odd", mk, ck),
    "uncovered": F.flow_uncovered,
}
NWAVES = {"uncovered/4 waves": 4}
_CLEAN = {}


def run(name, mut=None):
    ck, log = F.Check(), []
    HOST_CASES[name](_maker(mut, log, nwaves=NWAVES.get(name, 2048)), ck)
    for e in log:
        for msg in e.misses:
            ck.fail("window", f"{name}: {msg}")
        if e.disagree:
            ck.fail("bookkeeping", f"{name}: {len(e.disagree)} tiles, first: {e.disagree[0]}")
    return ck


def clean(name):
    if name not in _CLEAN:
        _CLEAN[name] = run(name)
    return _CLEAN[name]


# ---- the emulation inside the bound -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HOST_CASES))
def test_emulation_inside_the_bound(name):
    """Every family's bound holds, no word offset leaves its window, the census agrees with the emulation's bookkeeping and
    meets the GPU test's requirements (feat_check's NEED_* dicts, asserted by the flows as family `census`)."""
    ck = clean(name)
    print(f"\n[{name}] census", ck.census, "\nworst |emu - ref| / (2^-24 absref)", {k: round(v, 3) for k, v in sorted(ck.worst.items())})
    assert not ck.fails, ck.report()


def test_every_family_has_a_K_of_at_most_8():
    """K_FAMILY covers exactly the families the checker bounds, each a power of two of at most 8 (what K_BWD = K_FWD were)."""
    seen = set().union(*[set(clean(n).worst) for n in HOST_CASES])
    assert seen == set(R.K_FAMILY), set(R.K_FAMILY) ^ seen
    for f, k in R.K_FAMILY.items():
        assert 0 < k <= 8 and math.log2(k) == int(math.log2(k)), (f, k)
    assert not set(R.K_FAMILY) & set(R.EXACT_FAMILIES)
    worst = {f: max(clean(n).worst.get(f, 0.0) for n in HOST_CASES) for f in R.K_FAMILY}
    print("\nworst |emu - ref| / (2^-24 absref) over the host cases", {k: round(v, 3) for k, v in sorted(worst.items())})


# ---- the census -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["tiny", "odd"])
def test_census_without_a_gpu(grid):
    """The classes the GPU test requires of rays/<grid>, its colour-only launch, points/<grid> and flat/<grid>, from the cases
    alone (small_norm: from the restatement's own float64 |g|)."""
    for tag, case, need in ((f"{grid}/rays", F.record_mode_case(grid), F.NEED_RAYS),
                            (f"{grid}/points", F.explicit_points_case(grid), F.NEED_POINTS),
                            (f"{grid}/flat", F.flat_case(grid), F.NEED_FLAT)):
        p, valid = R.positions(case)
        nrm = R.forward_rows(case, p, valid)[2]
        gn = torch.zeros(case.tiles_all * 32, 4, dtype=torch.float64)
        gn[valid] = nrm
        _, counts = R.census(case, gnorm=gn.view(case.tiles_all, 32, 4).permute(0, 2, 1))
        assert all(counts[c] >= n for c, n in need.items()), (tag, need, counts)
        if "rays" in tag:
            case.grad_sdf = False
            _, counts = R.census(case)
            assert all(counts[c] >= n for c, n in F.NEED_RAYS_COLOUR.items()), (tag, counts)


# ---- the bar reach ----------------------------------------------------------------------------------------------------
def test_bar_reach():
    """feat_fwd_kernel<BAR> reads bar + o * 4 .. + 8 of a 7-cell bar unchecked: o = floor(ix[axis]) - b0 stays in 0..5 for all
    eight taps of each axis, with the kernel's own b0, on every valid sample of every host case's geometry and on `faces` for
    all four GRIDS dims (indices only), after the normalise / de-normalise round trip of tap_index."""
    cases = [F.record_mode_case(g) for g in ("tiny", "odd")] + [F.explicit_points_case(g) for g in ("tiny", "odd")]
    cases += [F.flat_case(g) for g in ("tiny", "odd")] + [F.groups_case(g) for g in ("tiny", "odd")]
    cases += [F.production_case((40, 40, 40)), F.partial_sources_case("grad4-0")]
    for dims in F.GRIDS.values():
        c = F._base_case((2, 2, 2), 1)
        c.dims = dims
        c.lo, c.hi = F._box(dims)
        pts = F.faces_points(c)
        c.pts, c.tiles_all = pts, (pts.shape[0] + 31) // 32
        cases.append(c)
    for c in cases:
        o = F.bar_reach(c)
        assert int(o.min()) >= 0 and int(o.max()) <= 5, (c.dims, int(o.min()), int(o.max()))
    assert max(int(F.bar_reach(c).max()) for c in cases) == 5             # (the sixth base cell is in use)


# ---- the mutants ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", list(E.MUTANTS))
def test_mutant_of_the_emulation_breaks_the_bound(mutant):
    want = set(E.MUTANTS[mutant])
    killed = set()
    hint = MUTANT_CASES.get(mutant, [])
    for name in hint + [n for n in HOST_CASES if n not in hint]:
        killed |= run(name, mutant).families() & want
        if killed == want:
            break
    assert killed == want, f"mutant `{mutant}` survives in {sorted(want - killed)}"


# the cases a mutant is tried on first (then all of HOST_CASES in order): only an order, to keep the file quick
MUTANT_CASES = {
    **{m: ["tiny/groups"] for m in ("group1_rows_96", "zero_pad_replicates", "tap_clamp_displaced_only")},
    **{m: ["tiny/flat"] for m in ("small_norm_projects", "small_norm_inv_norm", "gnorm_clamped", "points_jump_gt_4")},
    **{m: ["uncovered/4 waves"] for m in ("extra_on_covered_tiles_only", "uncovered_tile_reads_stale_rows", "clip_hi_off_by_one",
                                          "launch_range_sources_only")},
    "dsdf_extra_dropped": ["uncovered/4 waves", "abi/dsdf_out"],
    "value_tap_kept_with_dsdf_out": ["abi/dsdf_out"],
    **{m: ["abi/grad4-0"] for m in ("g4_scale_inverted", "g4_sign_x", "g4_corner_from_clamped_base")},
    "g4_zero_pad_ignored": ["abi/grad4-1"],
    "g4_self_drops_dsdf": ["abi/grad4-2"],
    **{m: ["abi/gap+dsdf_extra"] for m in ("anchor_unclamped", "colour_rows_of_source0")},
    "second_source_overwrites": ["abi/sources"],
    "hat_t_unrounded": ["tiny/faces"],
}


# ---- the checker itself -----------------------------------------------------------------------------------------------
def test_checker_reports_four_planted_errors_by_position():
    """A backend that returns the restatement's own values with one touched SDF cell moved by 2 K U absref, one untouched
    cell set to 1e-30, one forward row moved by 2 K U scale and one padding lane non-zero: four misses, each by position."""
    planted = {}

    class Planted(E.Emu):
        def fwd(self, radii=None):
            case = self.case
            p, valid = R.positions(case)
            val, scl, nrm, nabs = R.forward_rows(case, p, valid)
            n = case.tiles_all * 32
            X, G = torch.zeros(n, R.XROWS, dtype=torch.float64), torch.zeros(n, 4, dtype=torch.float64)
            X[valid], G[valid] = val, nrm
            jj = torch.nonzero(valid)[:, 0]
            r = R.ROW_FEAT + 9
            m = int(scl[:, r].argmax())
            X[jj[m], r] += 2 * R.K_FAMILY["stencil"] * R.U * scl[m, r]
            pad = int(torch.nonzero(~valid)[2, 0])
            X[pad, 50] = 1e-30
            planted.update(row=r, sample=int(jj[m]), pad=pad)
            T = case.tiles_all
            return X.view(T, 32, R.XROWS).permute(0, 2, 1), G.view(T, 32, 4).permute(0, 2, 1)

        def bwd(self, X, gn):
            case = self.case
            ref = R.scatter(case, X, gn)
            out, dsdf = super().bwd(X.float(), gn.float())
            for gid in out:
                g64 = torch.zeros(out[gid].numel(), dtype=torch.float64)
                if gid in ref.cells:
                    u, v, a = ref.cells[gid]
                    g64[u] = v
                    if gid == R.SDF_GID:
                        k = int(torch.argmax(a))
                        g64[u[k]] += 2 * R.K_FAMILY["sdf fit"] * R.U * a[k]
                        free = torch.ones(g64.numel(), dtype=torch.bool)
                        free[u] = False
                        z = int(torch.nonzero(free)[0, 0])
                        g64[z] = 1e-30
                        planted.update(cell=F._cell_name(case, gid, int(u[k])), zero=F._cell_name(case, gid, z))
                out[gid] = g64
            return out, dsdf

    ck = F.Check()
    case = F.flat_case("tiny")
    case.rec_ray = None
    case.pts = case.pts[:-5]                                  # five padding lanes at the end
    case.pt_sdf, case.pt_viewdirs = case.pt_sdf[:-5], case.pt_viewdirs[:-5]
    be = Planted(case)
    X, gn = F.check_forward("planted", case, be, None, ck)
    F.run("planted", case, be, dict(), ck, X, gn)
    assert len(ck.fails) == 4, ck.report()
    fams = [f for f, _ in ck.fails]
    assert sorted(fams) == ["padding", "sdf fit", "stencil", "untouched"], ck.report()
    msg = dict(ck.fails)
    assert f"forward row {planted['row']} of sample {planted['sample']} " in msg["stencil"] and "1 of" in msg["stencil"]
    assert f"(slot {planted['pad']})" in msg["padding"] and "rows [50]" in msg["padding"] and "1 such lanes" in msg["padding"]
    assert planted["cell"] in msg["sdf fit"] and "; 1 of" in msg["sdf fit"]
    assert planted["zero"] in msg["untouched"]
