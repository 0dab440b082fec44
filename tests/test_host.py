"""Host-side logic and the C-ABI surface, no GPU needed: the library loads and exports
every symbol of include/esr_hip.h, struct layouts agree with the C compiler, the drop-in
module reproduces the reference's initial state_dict, misuse fails loudly, and the
data-parallel sharding math is exact (world_size-2 gloo)."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_err


def test_library_loads_and_exports_every_header_symbol():
    from esr_nerf_amd import _lib, build
    build.build_lib()
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char \*)\s*\*?\s*(esr_\w+)\s*\(", header, re.M))
    assert len(declared) >= 25
    assert declared == set(_lib.EXPORTS)
    for name in declared:
        assert hasattr(L, name), name
    assert L.esr_abi_version() == _lib.ABI_VERSION
    assert b"gfx950" in L.esr_build_info()
    assert L.esr_mlp_packed_floats(0) > 0 and L.esr_mlp_packed_floats(7) < 0     # bad kind -> error code


# the test's own reading of the header's prototypes (not _lib's parser): return type, name, parameter list
PROTOTYPES = re.findall(r"^\s*(int|int64_t|const char \*)\s*(esr_\w+)\s*\(([^)]*)\)\s*;",
                        re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esr_hip.h")).read(), flags=re.S), re.M)
C_TYPES = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
           "double": ctypes.c_double, "const char *": ctypes.c_char_p}


@pytest.mark.parametrize("res, name, params", PROTOTYPES, ids=[p[1] for p in PROTOTYPES])
def test_every_entry_carries_the_signature_the_header_declares(res, name, params):
    """restype, arity and the exact type of every argument: scalars as declared, every pointer a c_void_p except the five that
    stay typed (the march struct, the two [host] boxes)."""
    from esr_nerf_amd import _lib
    params = [" ".join(p.split()) for p in params.split(",") if p.strip() != "void"]
    want = [ctypes.c_void_p if "*" in p else C_TYPES[p.rsplit(" ", 1)[0]] for p in params]
    typed = {"esr_march_count": (0, _lib.EsrMarch), "esr_march_fill": (0, _lib.EsrMarch), "esr_march_bwd": (0, _lib.EsrMarch),
             "esr_nonempty_mask": (4, ctypes.c_float), "esr_density_bounds": (4, ctypes.c_float)}
    if name in typed:
        i, target = typed[name]
        assert want[i] is ctypes.c_void_p
        want[i] = ctypes.POINTER(target)
    fn = getattr(_lib.lib(), name)
    assert fn.restype is C_TYPES[res]
    assert len(fn.argtypes) == len(params) and list(fn.argtypes) == want
    assert _lib.SIGNATURES[name] == (C_TYPES[res], want)


def test_a_bare_python_integer_reaches_an_int64_parameter_intact():
    """Both calls return from the host-side checks of esr_cd_hash_insert (nothing is launched, no pointer is read): a capacity of
    2^32 is a power of two only when all 64 bits arrive, and 2^31 keys are ESR_ECAP only when they arrive as 2^31."""
    from esr_nerf_amd import _lib
    L = _lib.lib()
    assert L.esr_cd_hash_insert(None, 0, 1 << 32, None, None, None) == 0
    p = ctypes.addressof((ctypes.c_int64 * 2)())
    assert L.esr_cd_hash_insert(p, 1 << 31, 1 << 32, p, None, None) == -2


def _lib_structs():
    """typedef name -> class, by the inverse of _lib's naming rule (EsrFeatBwdSrc -> esr_feat_bwd_src_t)"""
    from esr_nerf_amd import _lib
    return {re.sub(r"(?<!^)(?=[A-Z])", "_", c.__name__).lower() + "_t": c for c in vars(_lib).values()
            if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure}


def test_ctypes_structs_match_the_c_layout():
    """sizeof and every field's offsetof of every struct of the header, and the value of every integer #define, against the C
    compiler's."""
    from esr_nerf_amd import _lib
    structs = _lib_structs()
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    assert set(structs) == set(re.findall(r"^}\s*(esr_\w+_t)\s*;", header, re.M)) and len(structs) >= 23
    macros = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(ESR_\w+)[ \t]+\S", header, re.M)       # (ESR_HIP_H has no value)
    assert len(macros) >= 30 and len(set(macros)) == len(macros)
    exprs = [e for t, c in structs.items() for e in [f"sizeof({t})"] + [f"offsetof({t},{f[0]})" for f in c._fields_]]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "esr_hip.h"\nint main(){\n' +
           "".join(f'printf("%zu\\n",{e});\n' for e in exprs) +
           "".join(f'printf("%lld\\n",(long long)({m}));\n' for m in macros) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = dict(zip(exprs + macros, (int(v) for v in subprocess.check_output([exe]).split())))
    assert len(got) == len(exprs) + len(macros)
    for t, c in structs.items():
        assert got[f"sizeof({t})"] == ctypes.sizeof(c), t
        for f in c._fields_:
            assert got[f"offsetof({t},{f[0]})"] == getattr(c, f[0]).offset, (t, f[0])
    for m in macros:
        assert getattr(_lib, m[4:]) == got[m] and type(getattr(_lib, m[4:])) is int, m
    assert got["ESR_EINVAL"] == -1 and got["ESR_ECAP"] == -2


def _shape(ctype):
    """(element ctype, array lengths outermost first) of a field's ctypes type"""
    dims = []
    while issubclass(ctype, ctypes.Array):
        dims.append(ctype._length_)
        ctype = ctype._type_
    return ctype, dims


# the test's own reading of the header's structs (not _lib's parser): typedef name -> the text between its braces
STRUCT_BODIES = {t: body for body, t in re.findall(
    r"typedef\s+struct[^{;]*\{([^{}]*)\}\s*(esr_\w+_t)\s*;",
    re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esr_hip.h")).read(), flags=re.S))}


@pytest.mark.parametrize("typedef", sorted(STRUCT_BODIES))
def test_every_struct_carries_the_fields_the_header_declares(typedef):
    """Name, scalar / pointer / array, element type and array lengths of every field, in the header's order (offsets cannot tell
    `int32_t a; float b;` from `float a; int32_t b;`): scalars as declared, every pointer a c_void_p except esr_march_t.scene."""
    from esr_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    want = []
    for decl in STRUCT_BODIES[typedef].split(";"):
        words = decl.replace("const", " ").split(None, 1)
        if not words:
            continue
        for d in words[1].split(","):
            name = re.search(r"(\w+)\s*(?:\[|$)", d.strip()).group(1)
            dims = [int(n) if n.isdigit() else int(re.search(rf"#define\s+{n}\s+(\d+)", header).group(1))
                    for n in re.findall(r"\[\s*(\w+)\s*\]", d)]
            want.append((name, ctypes.c_void_p if "*" in d else C_TYPES[words[0]], dims))
    if typedef == "esr_march_t":
        assert want[0] == ("scene", ctypes.c_void_p, [])
        want[0] = ("scene", ctypes.POINTER(_lib.EsrScene), [])
    assert len(want) >= 2
    assert [(n, *_shape(t)) for n, t in _lib_structs()[typedef]._fields_] == want


def test_struct_fields_are_the_ones_the_hand_written_classes_had():
    """tests/golden/abi_struct_fields.json: names, order and types of the 22 classes _lib.py spelled out by hand before it
    derived them from the header (EsrBvhNode had none: the two tests above cover it)."""
    import json
    names = {ctypes.c_int32: "int32", ctypes.c_int64: "int64", ctypes.c_float: "float", ctypes.c_double: "double",
             ctypes.c_void_p: "void*"}

    def type_name(t):
        elem, dims = _shape(t)
        base = f"POINTER({elem._type_.__name__})" if issubclass(elem, ctypes._Pointer) else names[elem]
        return base + "".join(f"[{n}]" for n in dims)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_struct_fields.json")))
    got = {c.__name__: [[n, type_name(t)] for n, t in c._fields_] for c in _lib_structs().values()}
    assert len(golden) == 22 and set(got) == set(golden) | {"EsrBvhNode"}
    for name, fields in golden.items():
        assert got[name] == fields, name


@pytest.mark.parametrize("text, offender", [
    ("typedef struct esr_a { int32_t n; size_t bytes; } esr_a_t;", "bytes"),                  # a field type it does not know
    ("typedef struct esr_a { int32_t n : 3; } esr_a_t;", "int32_t n : 3"),                    # a declaration it cannot consume
    ("typedef struct esr_a { float v[ESR_NO_SUCH]; } esr_a_t;", "ESR_NO_SUCH"),               # a bound it has not read
    ("typedef struct esr_a { union { float f; int32_t i; } u; } esr_a_t;", "struct esr_a"),   # a typedef it cannot match
    ("struct esr_b;\ntypedef struct esr_a { float f; } esr_a_t;", "struct esr_b"),            # a struct no typedef accounts for
    ("typedef struct esr_a { float f; } esr_a_t;\nint esr_f(const esr_a_t *a);", "esr_march_t"),   # typed-pointer keys that name
])                                                                                                  # nothing in the header
def test_header_parser_fails_loudly(tmp_path, text, offender):
    from esr_nerf_amd import _lib
    h = tmp_path / "esr_hip.h"
    h.write_text("#define ESR_N 4\n" + text + "\n")
    with pytest.raises(RuntimeError, match=re.escape(offender)):
        _lib._parse_header(str(h))


def _cpu_model(**model_over):
    from esr_nerf_amd.config import fine_cfg
    from esr_nerf_amd.synthetic import init_slab_model, slab_scene
    from esr_nerf_amd.voxurff import VoxurfF
    sc = slab_scene("g16")
    cfg = fine_cfg("cpu")
    cfg.app.model.update(model_over)
    torch.manual_seed(0)
    np.random.seed(0)
    m = VoxurfF(cfg, sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max, sc.mask_alpha_init,
                sc.mask_density, sc.s_val, sc.num_voxels)
    return init_slab_model(m, sc), sc


def test_seeded_build_reproduces_reference_state_dict(golden_params):
    sd_ref, meta = golden_params
    m, _ = _cpu_model()
    sd = m.state_dict()
    assert list(sd.keys()) == list(sd_ref.keys())            # names AND order (checkpoint hand-off)
    for k in sd:
        assert sd[k].shape == sd_ref[k].shape, k
        assert torch.equal(sd[k], sd_ref[k]), k
    assert m.world_size.tolist() == meta["__world_size"].tolist()
    assert float(m.voxel_size) == float(meta["__voxel_size"])
    # logical layout is the reference's, storage is channels-last
    assert m.off_color.grid.shape == (1, 6, 32, 32, 8)
    assert m.off_color.grid.is_contiguous(memory_format=torch.channels_last_3d)
    # the optimizer addresses parameters by attribute name
    for name in ("off_color", "off_rgbnet", "emo_color", "emo_rgbnet", "sdf", "tonemapper"):
        assert hasattr(m, name)


def test_no_cpu_fallback_and_loud_config_errors():
    m, sc = _cpu_model()
    m.train()
    b = sc.batch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(rays_o=b["rays_o"], rays_d=b["rays_d"], viewdirs=b["viewdirs"], em_modes=b["em_modes"], s_val=20.0)
    with pytest.raises(NotImplementedError):
        _cpu_model(rgbnet_width=128)
    assert _cpu_model(neus_alpha="grad")[0].neus_alpha == "grad"        # both alpha modes of functions.py:45-105 exist
    with pytest.raises(ValueError):
        _cpu_model(neus_alpha="other")
    m.eval()                                   # image rendering is on the HIP path too: no CPU fallback either
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(rays_o=b["rays_o"], rays_d=b["rays_d"], viewdirs=b["viewdirs"], em_modes=0, pos_rt=torch.eye(3))
    from esr_nerf_amd import render_utils
    z = torch.zeros(3, 3)
    with pytest.raises(RuntimeError):
        render_utils.sample_pts_on_rays(z, z, z[0], z[0], 0.1, 1e9, 0.01)
    with pytest.raises(RuntimeError):
        render_utils.alpha2weight(torch.zeros(3), torch.zeros(3, dtype=torch.int64), 2)


def test_tv_regulariser_host_side():
    """density_total_variation: the plain SDF-TV branch (functions.py:34-42) is host-side torch; the smoothed-gradient
    branch is a HIP kernel pair and refuses CPU tensors (its parity test: tests/test_gpu_native_ops.py)."""
    m, _ = _cpu_model()
    tv = m.density_total_variation(sdf_tv=0.1, smooth_grad_tv=0)
    g, vs, mask = m.sdf.grid, m.voxel_size, m.nonempty_mask
    tv_sdf = sum(g.diff(dim=d).abs()[mask.narrow(d, 0, mask.shape[d] - 1) & mask.narrow(d, 1, mask.shape[d] - 1)].mean()
                 for d in (2, 3, 4)) / 3
    assert rel_err(tv.detach(), (tv_sdf / 2 / vs * 0.1).detach()) < 1e-6
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.density_total_variation(sdf_tv=0, smooth_grad_tv=0.05)


def test_shard_batch_partitions():
    from esr_nerf_amd.trainer import shard_batch
    b = {"a": torch.arange(10), "b": torch.arange(30).reshape(10, 3)}
    parts = [shard_batch(b, r, 3) for r in range(3)]
    assert torch.equal(torch.cat([p["a"] for p in parts]), b["a"])
    assert [len(p["a"]) for p in parts] == [3, 3, 4]


DP_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from esr_nerf_amd.config import fine_cfg
from esr_nerf_amd.synthetic import slab_scene
from esr_nerf_amd.trainer import shard_batch, dp_loss_weights
from oracle import fine_path as fp
import numpy as np
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
sc = slab_scene("g16", s_val=60.0, oblique=True)
z = np.load(os.path.join(sys.argv[1], "tests", "golden", "fine_g16_params.npz"))
sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
cfg = fine_cfg("cpu")
c = fp.make_consts(cfg.app.model, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max, sc.mask_alpha_init,
                   sc.mask_density, sc.near, sc.num_voxels)
def grads_of(batch, scale, w_ent):
    P = fp.params_from_state_dict(sd)
    res = fp.forward_training(P, c, batch, 60.0)
    loss, _ = fp.fine_loss(res, batch["rgbs"], weight_entropy_last=w_ent)
    (loss * scale).backward()
    keys = sorted(k for k, v in P.items() if v.grad is not None)
    return float(loss * scale), keys, torch.cat([P[k].grad.flatten() for k in keys])
n = sc.n_rays
local = shard_batch(sc.batch, rank, world)
scale, w_ent = dp_loss_weights(local["rays_o"].shape[0], n, rank == world - 1, 0.001)
loss, keys, flat = grads_of(local, scale, w_ent)
lt = torch.tensor([loss], dtype=torch.float64)
# the brick-sparse exchange (torch double of the brick kernels) must give the dense all-reduce's bits
from esr_nerf_amd.grad_sync import GridGradSync
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from brick_ops_double import TorchBrickOps
sparse = flat.float().clone()
sparse[: sparse.numel() // 3] = 0        # untouched bricks on both ranks
dense = sparse.clone()
sync = GridGradSync(dist.group.WORLD, ops=TorchBrickOps(), min_capacity=1)
sync.reduce(sparse)
sync.verify()
dist.all_reduce(dense)
assert torch.equal(sparse, dense) and sync.last["mode"] == "sparse", sync.last
# later steps size the brick list on the host from the previous step's count (no wait inside the exchange):
# same pattern again (fits), then a pattern with MORE dirty bricks than the capacity (overflow pass in verify())
for grow in (False, True):
    cur = flat.float().clone()
    if not grow:
        cur[: cur.numel() // 3] = 0
    else:
        cur[: cur.numel() // 8] = 0
        cur += (rank + 1) * 1e-3 * (cur != 0)
    want = cur.clone(); dist.all_reduce(want)
    sync.reduce(cur)
    sync.verify()
    assert torch.equal(cur, want), ("optimistic exchange", grow, sync.last)
    assert sync.last["mode"] == "sparse" and (("overflow" in sync.last) == grow), sync.last
sync2 = GridGradSync(dist.group.WORLD, dense_above=0.1, ops=TorchBrickOps())
again = flat.float().clone(); sync2.reduce(again)
ref2 = flat.float().clone(); dist.all_reduce(ref2)
assert torch.equal(again, ref2) and sync2.last["mode"] == "dense", sync2.last
dist.all_reduce(flat); dist.all_reduce(lt)
if rank == 0:
    full_loss, keys2, full = grads_of(sc.batch, 1.0, 0.001)
    assert keys == keys2
    err = float((flat - full).abs().max() / full.abs().max())
    print("DPRESULT", err, abs(float(lt) - full_loss))
dist.destroy_process_group()
'''


def test_data_parallel_sharding_is_exact_gloo_world2():
    """Two gloo ranks, ray shards of an oblique batch: all-reduced shard gradients (with the
    global-mean rescale and last-ray entropy ownership) equal the full-batch gradients."""
    with tempfile.TemporaryDirectory() as d:
        w = os.path.join(d, "w.py")
        open(w, "w").write(DP_WORKER)
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
        out = subprocess.run(
            [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
             "--master-addr", "127.0.0.1", "--master-port", "29517", w, ROOT],
            env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("DPRESULT")][0].split()
    assert float(line[1]) < 1e-5 and float(line[2]) < 1e-6, line


SHARD_WORKER = r'''
import math, os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from esr_nerf_amd.grad_sync import ShardedGrids
from esr_nerf_amd.modules import DenseGrid
from esr_nerf_amd.optimizer import ShardedGridAdam
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
ws = torch.tensor([6, 5, 4])
lo, hi = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
class M(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.sdf, self.off_color, self.emo_color = DenseGrid(1, ws, lo, hi), DenseGrid(6, ws, lo, hi), DenseGrid(6, ws, lo, hi)
        with torch.no_grad():
            for m_ in (self.sdf, self.off_color, self.emo_color):
                m_.grid.copy_(torch.randn(m_.grid.shape, generator=g))
model = M()
names = ["sdf", "off_color", "emo_color"]
lrs = {"sdf": 0.005, "off_color": 0.1, "emo_color": 0.05}
ref = {n: getattr(model, n).grid.detach().clone() for n in names}          # single-process reference copy
m_ref = {n: torch.zeros_like(v) for n, v in ref.items()}
v_ref = {n: torch.zeros_like(v) for n, v in ref.items()}

def torch_adam(p, g, m, v, lr, b1, b2, eps, step):                          # double of esr_adam_step (optimizer.py:183-228 arithmetic)
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    p.addcdiv_(m, (v.sqrt() / math.sqrt(1 - b2 ** step)).add_(eps), value=-(lr / (1 - b1 ** step)))

grids = ShardedGrids(model, names, dist.group.WORLD)
assert model.off_color.grid.is_contiguous(memory_format=torch.channels_last_3d) and model.off_color.grid.shape == (1, 6, 6, 5, 4)
assert model.sdf.grid.data_ptr() == grids.flat.data_ptr()                  # parameters are views of the flat buffer
assert grids.padded % (world * 128) == 0 and grids.shard * world == grids.padded
opt = ShardedGridAdam(grids, lrs, adam_fn=torch_adam)
for step in range(1, 4):
    # every rank's LOCAL gradients (storage order of the step's flat buffer: sdf | off [X,Y,Z,6] | emo [X,Y,Z,6])
    per_rank = [[torch.randn(ref[n].shape, generator=torch.Generator().manual_seed(1000 * step + 10 * r + i))
                 for i, n in enumerate(names)] for r in range(world)]
    mine = per_rank[rank]
    flat_grad = torch.cat([mine[0].flatten()] + [g_.permute(0, 2, 3, 4, 1).reshape(-1) for g_ in mine[1:]])
    grids.reduce_scatter(flat_grad)
    opt.step()
    opt.scale_lr(0.9)
    for i, n in enumerate(names):                                            # the single-process run on the summed gradient
        gsum = sum(per_rank[r][i] for r in range(world))
        torch_adam(ref[n], gsum, m_ref[n], v_ref[n], lrs[n] * 0.9 ** (step - 1), 0.9, 0.99, 1e-8, step)
    for n in names:
        err = float((getattr(model, n).grid.detach() - ref[n]).abs().max())
        assert err < 1e-6, (step, n, err)
assert opt.exp_avg.numel() == grids.shard                                   # moments exist for the owned shard only
# checkpoints: (a) the full state in the reference's per-parameter layout equals the single-process moments; (b) it loads
# back into a fresh sharded optimizer (any world size: every rank cuts its shard); (c) the shard-local state dict round-trips
full = opt.full_state()
for n in names:
    assert full["state"][n]["step"] == 3 and full["state"][n]["exp_avg"].is_contiguous()
    assert float((full["state"][n]["exp_avg"] - m_ref[n]).abs().max()) < 1e-6, n
    assert float((full["state"][n]["exp_avg_sq"] - v_ref[n]).abs().max()) < 1e-6, n
opt2 = ShardedGridAdam(grids, lrs, adam_fn=torch_adam)
opt2.load_full_state(full)
assert opt2.step_count == 3 and torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq)
assert all(abs(opt2.lr[n] - opt.lr[n]) < 1e-12 for n in names)
opt3 = ShardedGridAdam(grids, lrs, adam_fn=torch_adam)
opt3.load_state_dict(opt.state_dict())
assert opt3.step_count == 3 and torch.equal(opt3.exp_avg_sq, opt.exp_avg_sq)
bad = dict(opt.state_dict(), shard=(1, 2))
try:
    opt3.load_state_dict(bad)
    raise SystemExit("a foreign shard range must be refused")
except ValueError:
    pass
print("SHARDOK", rank, grids.shard, grids.padded)
dist.destroy_process_group()
'''


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_grid_adam_matches_single_process_gloo(world):
    """SURVEY 8(e) option 2 (ESR_GRAD_SYNC=shard): reduce-scatter of the dense-grid gradients, Adam on the owned
    shard, all-gather of the parameters -- three steps on 2 and 4 gloo ranks reproduce the single-process Adam on the
    summed gradients (torch double of esr_adam_step; colour grids channels-last inside the flat buffer)."""
    with tempfile.TemporaryDirectory() as d:
        w = os.path.join(d, "w.py")
        open(w, "w").write(SHARD_WORKER)
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
        out = subprocess.run(
            [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
             "--master-addr", "127.0.0.1", "--master-port", str(29520 + world), w, ROOT],
            env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.count("SHARDOK") == world, out.stdout[-2000:]


def test_optimizer_groups_freeze_and_no_cpu_fallback():
    """create_optimizer_or_freeze_model (app/utils/optimizer.py:11-60): one group per named attribute with
    lr > 0, lr == 0 freezes; the fused step refuses CPU parameters instead of falling back."""
    import torch.nn as nn
    from esr_nerf_amd.optimizer import create_optimizer_or_freeze_model

    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.a = nn.Linear(3, 2)
            self.b = nn.Parameter(torch.zeros(4))
            self.c = nn.Linear(2, 2)
    m = M()
    opt = create_optimizer_or_freeze_model(m, a=0.1, b=0.01, c=0.0, missing=1.0)
    assert set(opt.name2pg) == {"a", "b"} and opt.name2pg["a"]["lr"] == 0.1
    assert opt.defaults["betas"] == (0.9, 0.99)
    assert not any(p.requires_grad for p in m.c.parameters()) and m.b.requires_grad
    m.b.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()


def test_mesh_and_envmap_utilities():
    """extract_geometry's field sampler reproduces -sdf at the grid nodes; render_envmap matches the oracle's SG
    evaluation; without PyMCubes extract_geometry says so."""
    from esr_nerf_amd.config import lts_cfg
    from esr_nerf_amd.esrnerf import ESRNeRF
    from esr_nerf_amd.modules import extract_sdf_field
    from esr_nerf_amd.synthetic import init_slab_model, slab_scene
    from oracle import lts_path as lp
    sc = slab_scene("g16")
    torch.manual_seed(0)
    m = ESRNeRF(lts_cfg("cpu"), sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max, sc.mask_alpha_init,
                sc.mask_density, sc.s_val, sc.num_voxels)
    init_slab_model(m, sc)
    u = extract_sdf_field(m, resolution=9, batch_size=4, smooth=False)
    assert u.shape == (9, 9, 9)
    corner = float(-m.sdf.grid[0, 0, 0, 0, 0])
    assert abs(float(u[0, 0, 0]) - corner) < 1e-6 and abs(float(u[-1, -1, -1]) + float(m.sdf.grid[0, 0, -1, -1, -1])) < 1e-6
    img = m.render_envmap(6, 8)
    assert img.shape == (6, 8, 3)
    P = {"envmap.mus": m.envmap.mus.detach(), "envmap.lambdas": m.envmap.lambdas.detach(), "envmap.lobes": m.envmap.lobes.detach()}
    d = torch.tensor([[0.0, 0.0, 1.0]])                               # phi = 0: the first image row looks along +z
    assert rel_err(img[0, 0], lp.sg_envmap(P, d)[0]) < 1e-5
    try:
        import mcubes  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="PyMCubes"):
            m.extract_geometry(resolution=8)


def test_host_point_draw_equals_numpy_choice():
    """esr_host_choice_noreplace == np.random.choice(n, k, replace=False) of the legacy global generator, including
    the generator state it leaves behind (esrnerf.py:792 draws from that stream every step)."""
    import ctypes as C
    from esr_nerf_amd import _lib
    L = _lib.lib()

    def ours(n, k):
        st = np.random.get_state()
        key = np.ascontiguousarray(st[1], dtype=np.uint32).copy()
        pos = C.c_int32(int(st[2]))
        out = np.empty(k, dtype=np.int64)
        assert L.esr_host_choice_noreplace(key.ctypes.data_as(C.c_void_p), C.byref(pos), C.c_int64(n), C.c_int64(k),
                                           out.ctypes.data_as(C.c_void_p)) == 0
        np.random.set_state((st[0], key, pos.value, st[3], st[4]))
        return out

    for seed in range(4):
        for n, k in [(1, 1), (5, 3), (100, 100), (1000, 100), (80000, 100), (70001, 64)]:
            np.random.seed(seed); np.random.random(seed * 7)
            a = np.random.choice(n, k, replace=False); ra = np.random.random()
            np.random.seed(seed); np.random.random(seed * 7)
            b = ours(n, k); rb = np.random.random()
            assert np.array_equal(a, b) and ra == rb, (seed, n, k)
    assert L.esr_host_choice_noreplace(None, None, C.c_int64(3), C.c_int64(5), None) < 0


def test_point_draw_on_the_library_worker_equals_numpy_choice():
    """lts_engine._PointDraw (esr_host_choice_start / _wait: the draw on the library's worker thread, numpy's state checked
    out and back in) == np.random.choice of the legacy global generator, draw after draw; jobs queued behind one another
    come back in submission order with their own results."""
    import ctypes as C
    from esr_nerf_amd import _lib
    from esr_nerf_amd.lts_engine import _PointDraw
    ring = [None, None, 0, 0]
    for seed in range(3):
        for n, k in [(1, 1), (1000, 100), (80000, 100), (70001, 64), (5, 3)]:
            np.random.seed(seed); np.random.random(seed * 5)
            a = np.random.choice(n, k, replace=False); ra = np.random.random()
            np.random.seed(seed); np.random.random(seed * 5)
            b = _PointDraw(n, k, ring).result().numpy().copy(); rb = np.random.random()
            assert np.array_equal(a, b) and ra == rb, (seed, n, k)
    # two jobs in flight on separate states (the raw entry points): each handle returns its own draw
    L = _lib.lib()
    jobs = []
    for seed, (n, k) in enumerate([(50000, 10), (300, 300)]):
        st = np.random.RandomState(seed).get_state()
        key, pos, out, h = np.ascontiguousarray(st[1], dtype=np.uint32).copy(), C.c_int32(int(st[2])), np.empty(k, np.int64), C.c_void_p(0)
        assert L.esr_host_choice_start(C.c_void_p(key.ctypes.data), C.byref(pos), C.c_int64(n), C.c_int64(k),
                                       C.c_void_p(out.ctypes.data), C.byref(h)) == 0 and h.value
        jobs.append((seed, n, k, key, pos, out, h))
    for seed, n, k, key, pos, out, h in jobs:
        assert L.esr_host_choice_wait(h) == 0
        assert np.array_equal(out, np.random.RandomState(seed).choice(n, k, replace=False))
    h = C.c_void_p(0)
    assert L.esr_host_choice_start(None, None, C.c_int64(3), C.c_int64(5), None, C.byref(h)) < 0 and not h.value
    assert L.esr_host_choice_wait(None) < 0
    # a fork()ed child has the library's state but not its worker thread: the child's first job starts a new one
    import os
    np.random.seed(1)
    a = _PointDraw(1000, 10, ring).result().numpy().copy()
    pid = os.fork()
    if pid == 0:
        try:
            import signal
            signal.alarm(30)                   # (a stuck child ends itself: the parent sees a non-zero status)
            np.random.seed(1)
            b = _PointDraw(1000, 10, [None, None, 0, 0]).result().numpy().copy()
            os._exit(0 if np.array_equal(a, b) else 3)
        finally:
            os._exit(4)
    assert os.WEXITSTATUS(os.waitpid(pid, 0)[1]) == 0


def test_step_raises_a_deferred_march_overflow_on_the_next_step():
    """Data-parallel steps do not raise inside the step when a ray exceeded the march bound (the other ranks would hang in
    the exchange): the flag is reduced with the loss and every rank raises at the start of its next step."""
    from esr_nerf_amd.trainer import FineStep
    step = FineStep(model=None)                                     # (the overflow word needs no model and no GPU)
    step._check_overflow()                                          # nothing published yet: no-op
    lf = torch.tensor([0.25, 0.0])
    step._publish_overflow(lf)
    step._check_overflow()                                          # flag 0: fine
    step._publish_overflow(torch.tensor([0.25, 2.0]))               # two ranks saw an overflow
    with pytest.raises(RuntimeError, match="max_steps"):
        step._check_overflow()
    step._check_overflow()                                          # raised once, then cleared


def test_render_utils_shim_has_every_name_of_the_two_pybind_modules():
    """render_utils.cpp:170-184 (13 names) + total_variation.cpp:29-32 (2): the shim answers all of them -- also the ones the
    reference's own Python never calls (round 5: real launches, csrc/legacy_ops.hip; rounds 1-4 raised NotImplementedError) --
    and refuses CPU tensors the way the reference's CHECK_CUDA does."""
    import torch
    from esr_nerf_amd import render_utils
    names = ("infer_t_minmax", "infer_n_samples", "infer_ray_start_dir", "sample_pts_on_rays", "sample_ndc_pts_on_rays",
             "sample_bg_pts_on_rays", "maskcache_lookup", "raw2alpha", "raw2alpha_backward", "raw2alpha_nonuni",
             "raw2alpha_nonuni_backward", "alpha2weight", "alpha2weight_backward", "total_variation_add_grad",
             "total_variation_add_grad_new")
    for n in names:
        assert callable(getattr(render_utils, n)), n
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        render_utils.raw2alpha(torch.zeros(4), 0.0, 0.5)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        render_utils.maskcache_lookup(torch.zeros(2, 2, 2, dtype=torch.bool), torch.zeros(3, 3), torch.ones(3), torch.zeros(3))
    with pytest.raises(AttributeError):
        render_utils.no_such_op


def test_lts_point_share_adds_up_to_the_references_point_count():
    """``LtsStep(split_points=True)``: the ranks' surface-point counts add up to ``num_ltspts`` (lts.yaml: 100; 8 ranks used to
    get 12 each = 96) and their weights to 1, for every world size a node can have."""
    from esr_nerf_amd.trainer import lts_point_share
    for P in (100, 25, 7, 64):
        for world in (1, 2, 3, 4, 5, 6, 7, 8):
            if world > P:
                continue
            shares = [lts_point_share(P, world, r) for r in range(world)]
            assert sum(n for n, _ in shares) == P and abs(sum(w for _, w in shares) - 1.0) < 1e-12
            assert max(n for n, _ in shares) - min(n for n, _ in shares) <= 1
            assert all(abs(w - n / P) < 1e-15 for n, w in shares)


def test_default_exchange_form_by_world_size():
    """trainer.default_grid_sync: sparse for 2-4 ranks, dense from five on (and for one rank: nothing to exchange sparsely) -- the
    branch a node with 8 GPUs takes, which no GPU test can take here (this pool allows six processes per card)."""
    from esr_nerf_amd.trainer import default_grid_sync
    assert [default_grid_sync(w) for w in range(1, 9)] == ["dense", "sparse", "sparse", "sparse", "dense", "dense", "dense", "dense"]


def test_workspace_capacity_has_headroom_from_the_first_allocation():
    """lts_engine.Pass / fine_engine._Workspace: grow-only, 25 % headroom from the FIRST allocation on (round 6: a step that
    exceeded the first step's tile count by 1 % reallocated every buffer of a pass -- 12 hipMalloc calls, 82 ms)."""
    from esr_nerf_amd.lts_engine import Pass
    p = Pass("cpu", "t")
    p.ensure(1000)
    assert p.cap == 1266
    b = p.buf("x", rows=2)
    p.ensure(1200)                                   # within the headroom: the same buffers
    assert p.cap == 1266 and p.buf("x", rows=2) is b
    p.ensure(1300)                                   # beyond: larger, the old buffers dropped
    assert p.cap == int(1300 * 1.25) + 16 and p.buf("x", rows=2) is not b
    from esr_nerf_amd.fine_engine import _Workspace
    w = _Workspace("cpu")
    w.ensure(100)
    assert w.cap_tiles == 189
    x = w["X"]
    w.ensure(150)
    assert w.cap_tiles == 189 and w["X"] is x
