"""Checks on the generated gfx950 code of csrc/lpips.hip (compiled with the product's flags through esr_nerf_amd/build.py,
as tests/test_regroup_isa.py does; CPU only).  The file holds exactly the kernels listed here, and every one keeps
everything in registers: no scratch memory and no spills.  The convolution keeps its 33.8 KB of LDS and few enough
registers for the four workgroups per CU its grid cap counts on, and issues the f32 matrix instruction the header names."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_meta as km      # noqa: E402

SRC = os.path.join(ROOT, "esr_nerf_amd", "csrc", "lpips.hip")
KERNELS = ("conv_relu_kernel", "conv_pack_kernel", "maxpool_nhwc_kernel", "lpips_layer_kernel", "lp_sum_partials_kernel")


def test_lpips_kernels_use_no_scratch():
    meta = km.kernel_meta(km.asm_of(SRC))
    assert len(meta) == len(KERNELS), list(meta)
    for name in KERNELS:
        ks = [v for k, v in meta.items() if name in k]
        assert len(ks) == 1, (name, list(meta))
        k = ks[0]
        assert k.get("scratch", 0) == 0 and k.get("spill_v", 0) == 0 and k.get("spill_s", 0) == 0, (name, k)
    conv = [v for k, v in meta.items() if "conv_relu_kernel" in k][0]
    assert conv.get("vgpr", 999) + conv.get("agpr", 0) <= 128 and conv.get("lds", 1 << 20) * 4 <= 160 * 1024, conv


def test_convolution_runs_on_the_f32_matrix_instruction():
    asm = open(km.asm_of(SRC)).read()
    body = asm[asm.index("conv_relu_kernel"):]
    assert len(re.findall(r"^\s*v_mfma_f32_32x32x2_f32\b", body, re.M)) >= 16
    assert not re.search(r"^\s*(global|flat|buffer)_atomic", asm, re.M)
