"""The host side of the re-lighting edit-ray selection (esr_nerf_amd/relight.py), without a GPU: the numpy restatement
(tests/relight_ref.py) against the reference-generated fixture tests/golden/edit_rays.npz (tools/gen_edit_rays_golden.py),
the label attachment and filter bookkeeping on this package's ``RayGroupManager`` against the reference sampler's recorded
state, the header / ctypes declarations of the two entry points and the restated ``eval`` keys of cfg/app/pdra.yaml.

The clear-ray rule.  The reference projects with a BLAS matmul whose summation order is not the kernel's, so a ray whose
(u, v) lies within delta of a place where the outcome changes (relight_ref's clearance) is set aside; delta is 4 x the
largest |reference float32 (u, v) - float64 (u, v)| over the fixture, computed from the fixture, and at most 2 % of a case's
rays may be set aside.  The "integer" case projects exactly in float32 under any rounding order: nothing is set aside
there, the float32 restatement must give the reference's labels on every ray."""
import json
import os
import re

import numpy as np
import pytest
import torch

import relight_ref
from conftest import GOLDEN, ROOT

Z = np.load(os.path.join(GOLDEN, "edit_rays.npz"), allow_pickle=False)
CASES = relight_ref.cases(Z)
GENERIC = [c for c in CASES if c != "integer"]
LABELS = ("keep", "em_modes", "em_colors", "em_intensities")
UNCLEAR_CAP = 0.02


def test_fixture_covers_what_it_was_built_for():
    assert set(CASES) == {"wide", "tall", "integer"}
    sizes = {n: tuple(int(x) for x in relight_ref.case(Z, n)["image_size"]) for n in CASES}
    assert sizes["wide"][0] > sizes["wide"][1] and sizes["tall"][0] < sizes["tall"][1]           # (w, h): h < w and h > w
    modes = set()
    for n in CASES:
        c = relight_ref.case(Z, n)
        modes |= set(c["em_modes_cond"].tolist())
        assert len(c["cert_idxs_in"]) > 0 and not np.array_equal(c["uncert_idxs_in"], np.sort(c["uncert_idxs_in"]))
        frac = c["em_masks"][(c["em_masks"] > 0) & (c["em_masks"] < c["em_masks"].max())]
        assert frac.size > 0                                                                     # soft edges
        m = c["em_masks"]
        assert any((e > 0).any() for e in (m[:, :, 0], m[:, :, -1], m[:, 0], m[:, -1]))          # a mask on the border
        assert 0 < c["keep"].sum() < len(c["keep"])
    assert modes == {0, 1, 2, 3, 4}
    assert (relight_ref.case(Z, "wide")["esp"] == 0).all(1).sum() >= 50                          # points at the origin


@pytest.mark.parametrize("name", CASES)
def test_restated_dilation_equals_the_fixture(name):
    c = relight_ref.case(Z, name)
    assert np.array_equal(relight_ref.dilate(c["em_masks"], int(c["ks"])), c["dilated"])
    assert c["dilated"].dtype == np.float32


def test_the_even_window_is_anchored_like_opencv():
    m = np.zeros((1, 9, 30), np.float32)
    m[0, 4, 15] = 1.0
    d = relight_ref.dilate(m, 10)[0]
    ys, xs = np.nonzero(d)
    # a pixel at x reaches the outputs whose window -5 .. +4 contains it: x - 4 .. x + 5
    assert (xs.min(), xs.max()) == (11, 20) and (ys.min(), ys.max()) == (0, 8)


@pytest.mark.parametrize("name", GENERIC)
def test_restatement_gives_the_references_labels_on_every_clear_ray(name):
    delta = relight_ref.delta(Z)
    c = relight_ref.case(Z, name)
    r = relight_ref.case_label(c, np.float64)
    clear = r["clearance"] > delta
    print(f"{name}: delta {delta:.3e} px, {int((~clear).sum())} of {len(clear)} rays set aside ({100 * (1 - clear.mean()):.3f} %)")
    assert 0.0 < delta < 1e-2, delta
    assert 1.0 - clear.mean() <= UNCLEAR_CAP
    for k in LABELS:
        assert np.array_equal(np.asarray(r[k])[clear], c[k][clear]), k
    fin = np.isfinite(r["uv"]).all(1)
    assert np.abs(r["uv"][fin] - c["ref_uv"][fin]).max() <= delta / 4


def test_integer_case_projects_exactly_and_matches_on_every_ray():
    c = relight_ref.case(Z, "integer")
    r32, r64 = relight_ref.case_label(c, np.float32), relight_ref.case_label(c, np.float64)
    assert np.array_equal(r32["uv"], c["ref_uv"]) and np.array_equal(r64["uv"], c["ref_uv"].astype(np.float64))
    assert (c["ref_uv"] * 2 == np.round(c["ref_uv"] * 2)).all()                  # integers and a few exact halves
    for k in LABELS:
        assert np.array_equal(np.asarray(r32[k]), c[k]), k
    # the round trip matters: the definition evaluated at (u, v) itself differs from the reference on some of these rays
    differ = sum(int((np.asarray(r64[k]) != c[k]).reshape(len(c["keep"]), -1).any(1).sum()) for k in LABELS)
    print(f"integer: the float64 definition without grid_sample's round trip differs on {differ} label rows")
    assert (r64["clearance"][(np.asarray(r64["keep"]) != c["keep"])] == 0).all()


def _cpu_cfg():
    from esr_nerf_amd.config import AttrDict
    return AttrDict(system=dict(device="cpu", data_preload="cpu"))


@pytest.mark.parametrize("name", CASES)
def test_label_attachment_and_filter_leave_the_reference_samplers_state(name):
    from esr_nerf_amd.data import RayGroupManager
    from esr_nerf_amd.relight import attach_edit_labels
    c = relight_ref.case(Z, name)
    keys = ["rgbs", "rays_o", "rays_d", "viewdirs", "em_modes"]
    dataset = {k: torch.from_numpy(c[f"data/{k}"].copy()) for k in keys}
    own_modes = dataset["em_modes"].clone()
    s = RayGroupManager(_cpu_cfg(), dataset, list(keys), 64, 64, uncert_data_idxs=torch.from_numpy(c["uncert_idxs_in"]),
                        cert_data_idxs=torch.from_numpy(c["cert_idxs_in"]))
    if not torch.cuda.is_available():
        assert s.data["em_modes"] is dataset["em_modes"]                # the aliasing the attachment must respect
    attach_edit_labels(s, *(torch.from_numpy(c[k]) for k in LABELS))
    assert torch.equal(dataset["em_modes"], own_modes)
    assert s.keys == json.loads(str(c["keys"]))
    assert np.array_equal(s.uncert_data_idxs.numpy(), c["uncert_data_idxs"])
    assert np.array_equal(s.cert_data_idxs.numpy(), c["cert_data_idxs"])
    for k in s.keys:
        got_u, got_c = s.uncert(k).numpy(), s.cert(k).numpy()
        assert got_u.dtype == c[f"uncert/{k}"].dtype and np.array_equal(got_u, c[f"uncert/{k}"]), k
        assert got_c.dtype == c[f"cert/{k}"].dtype and np.array_equal(got_c, c[f"cert/{k}"]), k
    # what sample() hands out: the first rows of both groups, the edit keys among them
    b = s.sample()
    nu = min(64, len(c["uncert_data_idxs"]))
    for k in s.keys:
        want = np.concatenate([c[f"uncert/{k}"][:nu], c[f"cert/{k}"][:64]])
        assert np.array_equal(b[k].numpy(), want), k


def test_set_rows_refuses_nothing_and_changes_no_other_method():
    from esr_nerf_amd.data import RayGroupManager
    data = {"rays_o": torch.arange(12.0).reshape(4, 3), "em_modes": torch.tensor([1, 1, 0, 1])}
    s = RayGroupManager(_cpu_cfg(), data, ["rays_o", "em_modes"], 2, 2, uncert_data_idxs=torch.tensor([3, 0]),
                        cert_data_idxs=torch.tensor([1, 2]))
    s.set_rows("em_colors", s.uncert_data_idxs, torch.tensor([[0.5, 0.25], [1.0, 2.0]]), fill=0)
    assert s.data["em_colors"].tolist() == [[1.0, 2.0], [0.0, 0.0], [0.0, 0.0], [0.5, 0.25]]
    assert s.uncert("em_modes").tolist() == [1, 1] and s.stats() == dict(uncertain=2, certain=2, total=4)


def test_header_declares_the_entry_points_and_ctypes_agrees():
    from esr_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    # the names only: tests/test_host.py checks every entry's restype and argument types against the header text
    assert {"esr_mask_dilate", "esr_edit_label"} <= set(_lib.EXPORTS)
    m = re.search(r"#define ESR_RELIGHT_MAX_COND (\d+)", header)
    from esr_nerf_amd import relight
    assert int(m.group(1)) == relight.MAX_CONDITIONS
    assert relight.LIGHT_MODES == dict(off=0, on=1, i_change=2, c_change=3, ic_change=4)
