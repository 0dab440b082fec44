"""bench.py on one GPU: a plain run reports what its timed steps measured and runs nothing else; --full adds the sections
measured beside them (kernel breakdown and roofline, optimizer / zero-fill / TV timings, CPU baseline)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "loss"}
FULL_ONLY = {"kernel_ms_per_step_instrumented", "optimizer_step", "grad_zero_fill", "tv_terms", "cpu_baseline"}


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                          "--config", "small", *args],
                         env=dict(os.environ, OMP_NUM_THREADS="2"), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_reports_the_timed_steps_and_full_adds_the_rest():
    plain = _bench()
    assert HEADLINE <= set(plain) and plain["value"] > 0
    assert not (FULL_ONLY | {"roofline", "other_workloads"}) & set(plain), sorted(plain)
    full = _bench("--full", "--cpu-rays", "64", "--cpu-iters", "1")
    assert FULL_ONLY <= set(full), sorted(full)
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "config"):
        assert plain[k] == full[k], k
