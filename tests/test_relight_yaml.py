"""The ``eval`` keys of the reference's cfg/app/pdra.yaml that the re-lighting fine-tune reads (esr_nerf_amd/relight.py),
as esr_nerf_amd/config.py restates them, against the YAML tree itself (stored as data in tests/golden/reference_yaml.json
by oracle/gen_golden.py::gen_live) -- the ``eval`` half of tests/test_reference_yaml.py's comparison."""
import json
import os

from conftest import GOLDEN

with open(os.path.join(GOLDEN, "reference_yaml.json")) as _f:
    REF = json.load(_f)

RELIGHT_KEYS = {"mask_dilation_ks", "uncert_batch_size", "cert_batch_size", "n_iters", "lrs", "weight_lts", "batch_size"}


def _same(a, b):
    if isinstance(b, dict):
        return isinstance(a, dict) and set(a) == set(b) and all(_same(a[k], v) for k, v in b.items())
    try:
        return float(a) == float(b)                  # (PyYAML wrote `1e-05` as a string where OmegaConf reads a float)
    except (TypeError, ValueError):
        return a == b


def test_restated_eval_keys_equal_the_references_yaml():
    from esr_nerf_amd import config
    ref, mine = REF["app"]["pdra"]["eval"], config.PDRA_EVAL
    assert set(mine) == RELIGHT_KEYS
    wrong = {k: (ref.get(k), v) for k, v in mine.items() if k not in ref or not _same(ref[k], v)}
    assert not wrong, wrong


def test_lts_cfg_carries_the_eval_tree():
    from esr_nerf_amd.config import PDRA_EVAL, lts_cfg
    ev = lts_cfg("cpu").app.eval
    assert ev.mask_dilation_ks == 10 and ev.lrs.emo_rgbnet == 1e-05 and dict(ev, lrs=dict(ev.lrs)) == PDRA_EVAL
