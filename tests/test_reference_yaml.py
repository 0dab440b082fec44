"""B1's "drops into run.py under the existing Hydra configs", pinned: the reference's ACTUAL YAML tree
(cfg/app/{coarse,fine,lts,pdra}.yaml, stored as data in tests/golden/reference_yaml.json by oracle/gen_golden.py::gen_live)
against what esr_nerf_amd/config.py restates by hand for tests and bench.py, and the three renderers constructed from the
loaded ``app.model`` trees."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

with open(os.path.join(GOLDEN, "reference_yaml.json")) as _f:
    REF = json.load(_f)


def _load(name):
    return REF["app"][name]


def _same(a, b):
    """YAML 1.1 (PyYAML, which wrote the fixture) reads ``1e-5`` as a string where OmegaConf reads a float: numbers compare as numbers."""
    if isinstance(b, dict):
        return isinstance(a, dict) and all(k in a and _same(a[k], v) for k, v in b.items())
    if isinstance(b, (list, tuple)):
        return isinstance(a, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(b, bool) or b is None or isinstance(b, str) and not isinstance(a, str):
        return a == b
    try:
        return float(a) == float(b)
    except (TypeError, ValueError):
        return a == b


@pytest.mark.parametrize("yaml_name,section,restated", [
    ("fine", "model", "FINE_MODEL"), ("fine", "trainer", "FINE_TRAINER"),
    ("lts", "model", "LTS_MODEL"), ("lts", "trainer", "LTS_TRAINER"),
    ("pdra", "model", "LTS_MODEL"), ("pdra", "trainer", "PDRA_TRAINER"),
    ("coarse", "model", "COARSE_MODEL"), ("coarse", "trainer", "COARSE_TRAINER"),
])
def test_every_restated_key_equals_the_references_yaml(yaml_name, section, restated):
    from esr_nerf_amd import config
    ref, mine = _load(yaml_name)[section], getattr(config, restated)
    missing = [k for k in mine if k not in ref]
    assert not missing, (yaml_name, section, missing)
    wrong = {k: (ref[k], v) for k, v in mine.items() if not _same(ref[k], v)}
    assert not wrong, (yaml_name, section, wrong)


def _numeric(tree):
    """The loaded tree as OmegaConf would hand it over: exponent literals without a dot as floats."""
    out = {}
    for k, v in tree.items():
        if isinstance(v, dict):
            v = _numeric(v)
        elif isinstance(v, str):
            try:
                v = float(v)
            except ValueError:
                pass
        out[k] = v
    return out


def _cfg_from(yaml_name):
    from esr_nerf_amd.config import AttrDict
    app = _numeric(_load(yaml_name))
    return AttrDict(system=dict(device="cpu", debug=True, seed=0, tqdm_iters=10), app=app, data=dict(white_bg=True), global_step=0)


class _Reads(dict):
    """Records which keys of ``app.model`` a constructor reads (attribute access, as on a DictConfig)."""

    def __init__(self, d):
        super().__init__(d)
        self.read = set()

    def __getattr__(self, k):
        if k == "read":
            return object.__getattribute__(self, k)
        self.read.add(k)
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


@pytest.mark.parametrize("yaml_name,cls", [("fine", "VoxurfF"), ("lts", "ESRNeRF"), ("pdra", "ESRNeRF"), ("coarse", "VoxurfC")])
def test_renderers_construct_from_the_references_model_tree(yaml_name, cls):
    """VoxurfF / ESRNeRF / VoxurfC built from the YAML's own ``app.model`` (voxurff.py:61-77, esrnerf.py:75-101,
    voxurfc.py: the keys the reference's constructors read), on the CPU (construction needs no kernel): every key of the
    tree that the reference's model reads is read here, and none is missing."""
    from esr_nerf_amd.synthetic import slab_scene
    sc = slab_scene("g16")
    cfg = _cfg_from(yaml_name)
    model_tree = _Reads(cfg.app.model)
    cfg.app["model"] = model_tree
    torch.manual_seed(0)
    np.random.seed(0)
    if cls == "VoxurfC":
        from esr_nerf_amd.voxurfc import VoxurfC
        import inspect
        params = list(inspect.signature(VoxurfC.__init__).parameters)[2:]
        vals = dict(near=sc.near, far=sc.far, xyz_min=sc.xyz_min, xyz_max=sc.xyz_max, mask_xyz_min=sc.mask_xyz_min,
                    mask_xyz_max=sc.mask_xyz_max, mask_alpha_init=sc.mask_alpha_init, mask_density=sc.mask_density,
                    s_val=sc.s_val, num_voxles=sc.num_voxels, num_voxels=sc.num_voxels)
        m = VoxurfC(cfg, *[vals[p] for p in params if p in vals])
    else:
        mod = __import__("esr_nerf_amd." + {"VoxurfF": "voxurff", "ESRNeRF": "esrnerf"}[cls], fromlist=[cls])
        m = getattr(mod, cls)(cfg, sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max, sc.mask_alpha_init,
                              sc.mask_density, sc.s_val, sc.num_voxels)
    assert sum(p.numel() for p in m.parameters()) > 0
    unread = set(model_tree) - model_tree.read
    # A key of the tree the constructor never looked at would be a setting silently ignored -- unless the reference ignores
    # it too (pdra.yaml:41 `ray_sampling_eval` occurs in no .py file of the reference; the fixture lists, per tree, the
    # model keys that occur as text anywhere in the reference's Python sources)
    mentioned = set(REF["model_keys_in_reference_py"][yaml_name])
    ignored_here_only = sorted(k for k in unread if k in mentioned)
    assert not ignored_here_only, (yaml_name, cls, ignored_here_only)
