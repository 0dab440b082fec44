"""Does every product source compile to the same device code here as in another tree (the gate of a kernel refactor)?
   python tools/asm_same.py OTHER_TREE [march.hip ...]      (CPU only; default: every csrc/*.hip of this tree)
Each tree compiles with its own esr_nerf_amd/build.py (device_asm: its flags, its _obj/), OTHER_TREE in a child process
started there.  The lines naming the per-translation-unit `__hip_cuid_<hash>` symbol are dropped, the rest is compared as
text: `same` or `DIFFERENT (first differing line ...)` per file, exit status 1 on any difference."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from esr_nerf_amd.build import device_asm, sources      # noqa: E402


def asm_lines(path):
    return [l for l in open(path).read().splitlines() if "__hip_cuid_" not in l]


if __name__ == "__main__":
    if len(sys.argv) < 2 or not os.path.isdir(sys.argv[1]):
        sys.exit(__doc__)
    other, files = os.path.abspath(sys.argv[1]), sys.argv[2:] or sources()
    child = "import sys\nfrom esr_nerf_amd.build import device_asm\nfor f in sys.argv[1:]: print(device_asm(f))"
    theirs = subprocess.run([sys.executable, "-c", child, *files], cwd=other, capture_output=True, text=True)
    if theirs.returncode != 0:
        sys.exit(f"{other}: device_asm failed\n{theirs.stderr}")
    bad = 0
    for f, their_path in zip(files, theirs.stdout.splitlines()):
        a, b = asm_lines(device_asm(f)), asm_lines(their_path)
        diff = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
        if diff is None:
            print(f"{f:18s} same")
        else:
            bad += 1
            print(f"{f:18s} DIFFERENT (first differing line {diff + 1} after the drop: {a[diff:diff + 1]} | {b[diff:diff + 1]})")
    sys.exit(1 if bad else 0)
