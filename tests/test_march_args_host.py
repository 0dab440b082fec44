"""Argument checks of esr_march_count / _fill / _bwd (include/esr_hip.h: esr_march_t) that end before any launch: the NULL
struct, the NULL scene, a negative ray count, a count without a plan, every refused flag / field combination, and the
sixteen legal shapes with no rays.  (The missing-pointer rule needs n_rays > 0, where a wrong check would launch: it is
read against the kernel, not run.)"""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT

EINVAL = -1
X = 0x1000                              # a non-NULL address: never dereferenced, no pass launches with n_rays == 0
PASSES = ("count", "fill", "bwd")


@pytest.fixture(scope="module")
def lib():
    from esr_nerf_amd import _lib, build
    build.build_lib()
    return _lib, _lib.lib()


def _args(lib, n_rays=0, **fields):
    _lib, _ = lib
    scene = _lib.EsrScene(max_steps=100)
    return _lib.EsrMarch(scene=C.pointer(scene), n_rays=n_rays, plan=X, **fields)


def _call(lib, which, a):
    return getattr(lib[1], "esr_march_" + which)(a, None)


def test_struct_matches_the_c_layout(lib):
    _lib, _ = lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "esr_hip.h"\nint main(){printf("%zu %zu %zu %zu %d %d",'
           'sizeof(esr_march_t),offsetof(esr_march_t,flags),offsetof(esr_march_t,accumulate),offsetof(esr_march_t,cache),'
           'ESR_MARCH_COARSE,ESR_MARCH_GRAD_ALPHA);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    E = _lib.EsrMarch
    assert got == [C.sizeof(E), E.flags.offset, E.accumulate.offset, E.cache.offset, _lib.MARCH_COARSE, _lib.MARCH_GRAD_ALPHA]


@pytest.mark.parametrize("which", PASSES)
def test_null_struct_null_scene_negative_count(lib, which):
    assert _call(lib, which, None) == EINVAL
    a = _args(lib)
    a.scene = None
    assert _call(lib, which, a) == EINVAL
    assert _call(lib, which, _args(lib, n_rays=-1)) == EINVAL


def test_count_needs_a_plan(lib):
    a = _args(lib)
    a.plan = None
    assert _call(lib, "count", a) == EINVAL
    assert _call(lib, "fill", a) == 0 and _call(lib, "bwd", a) == 0


REFUSED = [dict(flags=f, **{k: X}) for k in ("cache", "dsdf_rec") for f in (1, 2, 3)] + \
          [dict(flags=f, **{k: X}) for k in ("gg", "grad_gg") for f in (0, 1, 2)] + \
          [dict(flags=4), dict(flags=7), dict(flags=-1), dict(flags=1 << 16)]


@pytest.mark.parametrize("which", PASSES)
@pytest.mark.parametrize("fields", REFUSED, ids=lambda f: ",".join(f"{k}={v}" for k, v in f.items()))
def test_combinations_no_march_offers_are_refused_before_the_empty_shortcut(lib, which, fields):
    assert _call(lib, which, _args(lib, **fields)) == EINVAL


# (pass, flags, fields): plain / cached / grad-alpha / coarse / coarse grad-alpha x count, fill, bwd, and the fine backward
# with dsdf_rec -- the sixteen entry points the three replace
LEGAL = [(w, f, {}) for f in (0, 1, 2, 3) for w in PASSES] + [(w, 0, dict(cache=X)) for w in PASSES] + \
        [("bwd", 0, dict(dsdf_rec=X))]


@pytest.mark.parametrize("which,flags,fields", LEGAL, ids=lambda v: str(v))
def test_the_sixteen_legal_shapes_return_0_without_rays(lib, which, flags, fields):
    assert len(LEGAL) == 16
    if flags == 3:
        fields = dict(fields, gg=X, grad_gg=X)
    assert _call(lib, which, _args(lib, flags=flags, **fields)) == 0
    assert _call(lib, which, _args(lib, flags=flags)) == 0                       # (with no rays no field is required)
