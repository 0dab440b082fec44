"""The generated gfx950 code of csrc/raster.hip (compiled with the product's flags through esr_nerf_amd/build.py, as
tests/test_regroup_isa.py does; CPU only): the file holds exactly the kernels listed here and none of them uses scratch
memory -- the per-face set-up (nine projected coordinates, three depths, the box) stays in registers on both paths.
Scratch is all this test looks at."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_meta as km      # noqa: E402

KERNELS = ("raster_small_kernel", "raster_large_kernel", "raster_resolve_kernel", "source_masks_kernel")


def test_raster_kernels_use_no_scratch():
    meta = km.kernel_meta(km.asm_of(os.path.join(ROOT, "esr_nerf_amd", "csrc", "raster.hip")))
    assert len(meta) == len(KERNELS), list(meta)
    for name in KERNELS:
        ks = [v for k, v in meta.items() if name in k]
        assert len(ks) == 1, (name, list(meta))
        k = ks[0]
        assert k.get("scratch", 0) == 0 and k.get("spill_v", 0) == 0 and k.get("spill_s", 0) == 0, (name, k)
