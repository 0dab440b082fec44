"""Checks on the generated gfx950 code of csrc/regroup.hip (compiled with the product's flags through esr_nerf_amd/build.py,
as tests/test_relight_isa.py does; CPU only).  The file holds exactly the kernels listed here, and every one keeps everything
in registers: no scratch memory, no spills, and few enough vector registers for the eight waves per SIMD the design note
claims (at most 64 registers per lane).  Registers and scratch are all this test looks at."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_meta as km      # noqa: E402

EIGHT_WAVES = 64              # allocated vector + accumulation registers per lane that still admit 8 waves per SIMD
KERNELS = ("regroup_stats_init_kernel", "emit_decide_kernel", "emit_decide_bits_kernel", "flags_pack_kernel", "flags_unpack_kernel",
           "flag_count_bits_kernel", "flag_scan_kernel", "index_partition_bits_kernel", "regroup_stats_merge_kernel")


def test_regroup_kernels_use_no_scratch_and_fit_eight_waves():
    meta = km.kernel_meta(km.asm_of(os.path.join(ROOT, "esr_nerf_amd", "csrc", "regroup.hip")))
    assert len(meta) == len(KERNELS), list(meta)
    for name in KERNELS:
        ks = [v for k, v in meta.items() if name in k]
        assert len(ks) == 1, (name, list(meta))
        k = ks[0]
        assert k.get("scratch", 0) == 0 and k.get("spill_v", 0) == 0 and k.get("spill_s", 0) == 0, (name, k)
        assert k.get("vgpr", 999) + k.get("agpr", 0) <= EIGHT_WAVES and k.get("occupancy") == 8, (name, k)
