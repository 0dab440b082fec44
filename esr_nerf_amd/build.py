"""Build libesr_hip.so (in-tree) with hipcc for gfx950; the one owner of the compile command.

``python -m esr_nerf_amd.build [--force]`` or ``__graft_entry__.build()``.  hipcc
cross-compiles without a GPU; the built library is git-ignored.  Everything else that
compiles a product source uses ``hipcc_cmd`` (the product's flags for that source):

    python -m esr_nerf_amd.build --variant NAME SRC [FLAG ...]   tools/_variants/NAME.so: the in-tree library with
                                                                 csrc/SRC recompiled under the additional flags (an A/B
                                                                 build, loaded with ESR_LIB_PATH)
    python -m esr_nerf_amd.build --flags SRC                     the product's flags for csrc/SRC (for harnesses that
                                                                 #include it: tools/ubench/build.sh)
    device_asm(SRC)                                              device assembly of csrc/SRC (tools/kernel_meta.py,
                                                                 tools/isa_waits.py, tests/test_isa.py)
"""
from __future__ import annotations

import concurrent.futures as cf
import hashlib
import os
import shlex
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "_obj")
LIB = os.path.join(HERE, "libesr_hip.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "esr_hip.h")
VARIANTS = os.path.join(os.path.dirname(HERE), "tools", "_variants")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"
# NO packed-fp32 arithmetic (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32 / v_pk_mov_b32) in any product kernel: the target feature is
# switched off (`-target-feature -packed-fp32-ops`): whatever builds <2 x float> operations -- the SLP vectoriser, the loop
# vectoriser, a sum of two f32x4 accumulators in the source -- is scalarised by the backend.
# Why (round 6, DESIGN 5 "packed fp32"): on this hardware a packed-fp32 instruction whose op_sel reads a HIGH half for the low result
# (v_pk_add_f32 / v_pk_mul_f32 ... op_sel:[0,1]) returns wrong results in lanes 48-63 while ANOTHER wave of the same SIMD alternates
# MFMAs with op_sel'd v_fma_mix_f32 -- which is what the split-fp16 kernels do.  A standalone kernel showed it with nothing of
# this library involved (6.9 M wrong results in 3000 launches, none in any other lane quarter, none beside any other load:
# profiles/r06_pk_beside_mfma.txt);
# esr_expgrad_fwd, whose x / y interpolation weights the SLP vectoriser had packed exactly so, returned wrong rows in 44 % of its
# launches beside the C2 step and in 1.5 % of the light-transport steps of two ranks sharing a card (profiles/r06_packed_fp32_lanes.txt).
# Cost: none -- three builds alternating on one box, C2 step: packed 2.066-2.083 ms, this build 2.053-2.070 ms, this build without
# the SLP vectoriser as well 2.091-2.110 ms (the vectoriser's merged loads and stores are worth keeping; C4 / C3 bf16: within 1 %
# of each other: profiles/r06_ab_packed_fp32_builds.txt).  tests/test_isa.py asserts that no kernel of the library holds a
# packed-fp32 instruction.
NO_PACKED_FP32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-fvisibility=hidden",
         "-Wall", "-Wno-unused-function", "-fno-fast-math", *NO_PACKED_FP32]


# per-source flags.
# mlp_split.hip, which runs ONE wave per SIMD on ~430 registers: `-mllvm -amdgpu-mfma-vgpr-form=1` keeps the MFMA accumulators in
# the VGPR half -- the epilogue's vector instructions read them there instead of through v_accvgpr_read: 600 -> 367 accumulation-
# register moves per tile group in the radiance forward (5441 -> 5198 instructions), 466 -> 234 in the input gradients (4556 ->
# 4321).  Round 4 measured the flag slower on that round's kernel (three accumulator sets: the planes' traffic moved to
# v_accvgpr_write, 0.705 -> 0.72 ms); on today's kernels, three alternating rounds on one box: radiance forward 0.491-0.495 ->
# 0.479-0.483 ms, C2 step 1.981-1.994 -> 1.972-1.983 ms (round 6; the same flag on mlp.hip moves nothing at C3 / C4 / C5).
# tone_wgrad.hip: the SLP vectoriser pairs the per-lane fp32 sums of the weight-gradient kernels up in register PAIRS -- 150 register
# moves per tile and 100+ more live registers in tone_wgrad_split_t_kernel (367 registers, or 320 bytes of scratch at two waves per
# SIMD; 194 registers and no moves without it: round 6).
EXTRA = {"tone_wgrad.hip": ["-fno-slp-vectorize"], "mlp_split.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]}


def hipcc_cmd(src, extra=()):
    """hipcc with the product's flags for csrc/SRC (FLAGS + EXTRA[src]), then the caller's additional flags."""
    return [HIPCC, *FLAGS, *EXTRA.get(src, []), *extra]


def sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


def _make(src, out, args):
    """Compile csrc/SRC into `out` with the product's flags + `args`, unless out's stamp shows it was built from these sources
    with these flags (paths are left out of the stamp: a moved checkout stays built).  Returns whether it compiled."""
    h = hashlib.sha1(" ".join(hipcc_cmd(src, args)[1:]).encode())
    for p in sorted([os.path.join(CSRC, src), HEADER] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]):
        with open(p, "rb") as f:
            h.update(f.read())
    stamp, sfile = h.hexdigest(), out + ".stamp"
    if os.path.exists(out) and os.path.exists(sfile) and open(sfile).read() == stamp:
        return False
    r = subprocess.run([*hipcc_cmd(src, args), os.path.join(CSRC, src), "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
    # (the host pass of the same command does not know the device feature: "'-packed-fp32-ops' is not a recognized feature for
    #  this target (ignoring feature)", once per function; hipcc's own '--hip-link' is unused by a -S compile -- both dropped;
    #  everything else the compiler says is passed on)
    noise = ("'-packed-fp32-ops' is not a recognized feature", "argument unused during compilation: '--hip-link'")
    err = "\n".join(l for l in r.stderr.splitlines() if not any(n in l for n in noise))
    if err.strip():
        sys.stderr.write(err + "\n")
    with open(sfile, "w") as f:
        f.write(stamp)
    return True


def _compile(src, extra=(), obj=None):
    obj = obj or os.path.join(OBJ, src[:-4] + ".o")
    return obj, _make(src, obj, [*extra, "-c"])


def _link(objs, lib):
    r = subprocess.run([HIPCC, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", lib, *objs], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")


def build_lib(force: bool = False, jobs: int = 4) -> str:
    os.makedirs(OBJ, exist_ok=True)
    if force:
        for f in os.listdir(OBJ):
            os.remove(os.path.join(OBJ, f))
    with cf.ThreadPoolExecutor(max_workers=jobs) as ex:
        res = list(ex.map(_compile, sources()))
    if any(changed for _, changed in res) or not os.path.exists(LIB):
        _link([o for o, _ in res], LIB)
    return LIB


def build_variant(name, src, extra=()) -> str:
    """tools/_variants/NAME.so: the in-tree objects with csrc/SRC recompiled (into NAME.o) under the additional flags."""
    if src not in sources():
        raise ValueError(f"no source csrc/{src}")
    build_lib()
    os.makedirs(VARIANTS, exist_ok=True)
    obj, _ = _compile(src, extra, os.path.join(VARIANTS, name + ".o"))
    lib = os.path.join(VARIANTS, name + ".so")
    _link([obj if s == src else os.path.join(OBJ, s[:-4] + ".o") for s in sources()], lib)
    return lib


def device_asm(src) -> str:
    """Device assembly of csrc/SRC as the product compiles it: esr_nerf_amd/_obj/<name>.s for <name>.hip."""
    os.makedirs(OBJ, exist_ok=True)
    out = os.path.join(OBJ, src[:-4] + ".s")
    _make(src, out, ["-S", "--cuda-device-only"])
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--variant"] and len(args) >= 3:
        print(build_variant(args[1], args[2], args[3:]))
    elif args[:1] == ["--flags"] and len(args) == 2:
        print(shlex.join(hipcc_cmd(args[1])[1:]))
    elif args in ([], ["--force"]):
        print(build_lib(force=bool(args)))
    else:
        sys.exit(__doc__)
