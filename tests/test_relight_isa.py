"""Checks on the generated gfx950 code of csrc/relight.hip (compiled with the product's flags through esr_nerf_amd/build.py,
as tests/test_isa.py does; CPU only).  Both kernels keep everything in registers: no scratch memory, and few enough
vector registers for the eight waves per SIMD the design note claims (at most 64 registers per lane)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_meta as km      # noqa: E402

EIGHT_WAVES = 64              # allocated vector + accumulation registers per lane that still admit 8 waves per SIMD


def _asm():
    return km.asm_of(os.path.join(ROOT, "esr_nerf_amd", "csrc", "relight.hip"))


def test_relight_kernels_use_no_scratch_and_fit_eight_waves():
    meta = km.kernel_meta(_asm())
    for name in ("mask_dilate_kernel", "edit_label_kernel"):
        ks = [v for k, v in meta.items() if name in k]
        assert len(ks) == 1, (name, list(meta))
        k = ks[0]
        assert k.get("scratch", 0) == 0 and k.get("spill_v", 0) == 0 and k.get("spill_s", 0) == 0, (name, k)
        assert k.get("vgpr", 999) + k.get("agpr", 0) <= EIGHT_WAVES and k.get("occupancy") == 8, (name, k)


def test_label_kernel_is_a_plain_streaming_kernel():
    """No atomics, no LDS, no packed-fp32 arithmetic; every output leaves through ordinary vector stores."""
    txt = open(_asm()).read()
    body = txt[txt.index("edit_label_kernel"):]
    body = body[: body.index(".Lfunc_end")]
    ops = re.findall(r"^\s+([a-z]\w+)", body, re.M)
    assert not [o for o in ops if "atomic" in o or o.startswith("ds_") or o.startswith("v_pk_")], sorted(set(ops))
    stores = [o for o in ops if "store" in o]
    assert stores and all(o.startswith(("global_store", "buffer_store", "flat_store")) for o in stores), sorted(set(stores))
