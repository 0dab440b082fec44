"""The generated gfx950 code of csrc/surfpath_is.hip (compiled with the product's flags through esr_nerf_amd/build.py, as
tests/test_surfpath_isa.py does; CPU only): the file holds exactly the two kernels listed here, neither uses scratch memory or
spills a register -- the path's vertex, its throughput, the nine sums, the walk, and for a few instructions the frame and the
binary64 exp and log stay in registers -- and the LDS is at most the lobe table (7 * 64 floats).  That is all this test looks at."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_meta as km      # noqa: E402

KERNELS = ("surfpath_is_reflect_kernel", "surfpath_is_irradiance_kernel")
LOBE_TABLE = 7 * 64 * 4


def test_surfpath_is_kernels_use_no_scratch():
    meta = km.kernel_meta(km.asm_of(os.path.join(ROOT, "esr_nerf_amd", "csrc", "surfpath_is.hip")))
    assert len(meta) == len(KERNELS), list(meta)
    for name in KERNELS:
        ks = [v for k, v in meta.items() if name in k]
        assert len(ks) == 1, (name, list(meta))
        k = ks[0]
        assert k.get("scratch", 0) == 0 and k.get("spill_v", 0) == 0 and k.get("spill_s", 0) == 0, (name, k)
        assert k.get("lds", 0) <= LOBE_TABLE, (name, k)
        print(name, k)
