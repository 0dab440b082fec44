"""Checks on the generated gfx950 code of csrc/rayfilter.hip (compiled with the product's flags through
esr_nerf_amd/build.py, as tests/test_relight_isa.py does; CPU only).  Both sampling modes keep everything in registers: no
scratch, no spills, few enough vector registers for eight waves per SIMD; no LDS, no atomics, no packed-fp32 arithmetic;
the flags leave through ordinary vector stores."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_meta as km      # noqa: E402

EIGHT_WAVES = 64              # allocated vector + accumulation registers per lane that still admit 8 waves per SIMD


def _asm():
    return km.asm_of(os.path.join(ROOT, "esr_nerf_amd", "csrc", "rayfilter.hip"))


def test_filter_kernels_use_no_scratch_and_fit_eight_waves():
    meta = {k: v for k, v in km.kernel_meta(_asm()).items() if "ray_filter_kernel" in k}
    assert len(meta) == 2, list(meta)                       # the march and the fixed instantiation
    for name, k in meta.items():
        assert k.get("scratch", 0) == 0 and k.get("spill_v", 0) == 0 and k.get("spill_s", 0) == 0, (name, k)
        assert k.get("lds", 0) == 0, (name, k)
        assert k.get("vgpr", 999) + k.get("agpr", 0) <= EIGHT_WAVES and k.get("occupancy") == 8, (name, k)


def test_filter_kernels_are_plain_gather_kernels():
    txt = open(_asm()).read()
    bodies = re.findall(r"^(_Z\w*ray_filter_kernel\w*):[^\n]*\n(.*?)\.Lfunc_end", txt, re.M | re.S)
    assert len(bodies) == 2, [b[0] for b in bodies]
    for name, body in bodies:
        ops = re.findall(r"^\s+([a-z]\w+)", body, re.M)
        assert not [o for o in ops if "atomic" in o or o.startswith("ds_") or o.startswith("v_pk_")], (name, sorted(set(ops)))
        stores = [o for o in ops if "store" in o]
        assert stores and all(o.startswith(("global_store", "buffer_store")) for o in stores), (name, sorted(set(stores)))
