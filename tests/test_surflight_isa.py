"""The generated gfx950 code of csrc/surflight.hip (compiled with the product's flags through esr_nerf_amd/build.py, as
tests/test_raycast_isa.py does; CPU only): the file holds exactly the kernels listed here and none of them uses scratch
memory or spills a register -- the point, the slot's geometric term and the whole walk stay in registers.  That is all this
test looks at."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_meta as km      # noqa: E402

KERNELS = ("surflight_reflect_kernel", "surflight_irradiance_kernel")


def test_surflight_kernels_use_no_scratch():
    meta = km.kernel_meta(km.asm_of(os.path.join(ROOT, "esr_nerf_amd", "csrc", "surflight.hip")))
    assert len(meta) == len(KERNELS), list(meta)
    for name in KERNELS:
        ks = [v for k, v in meta.items() if name in k]
        assert len(ks) == 1, (name, list(meta))
        k = ks[0]
        assert k.get("scratch", 0) == 0 and k.get("spill_v", 0) == 0 and k.get("spill_s", 0) == 0 and k.get("lds", 0) == 0, (name, k)
