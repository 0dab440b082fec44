"""The generated gfx950 code of csrc/atlas.hip (compiled with the product's flags through esr_nerf_amd/build.py, as
tests/test_surfenv_isa.py does; CPU only): the file holds exactly the kernels listed here, and none of them uses scratch memory
or spills a register -- the group tables are read from the kernel arguments, not copied into an indexed array.  That is all this
test looks at."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_meta as km      # noqa: E402

KERNELS = ("atlas_levels_kernel", "atlas_charts_kernel", "atlas_texels_kernel", "atlas_sample_kernel")


def test_atlas_kernels_use_no_scratch():
    meta = km.kernel_meta(km.asm_of(os.path.join(ROOT, "esr_nerf_amd", "csrc", "atlas.hip")))
    assert len(meta) == len(KERNELS), list(meta)
    for name in KERNELS:
        ks = [v for k, v in meta.items() if name in k]
        assert len(ks) == 1, (name, list(meta))
        k = ks[0]
        assert k.get("scratch", 0) == 0 and k.get("spill_v", 0) == 0 and k.get("spill_s", 0) == 0, (name, k)
