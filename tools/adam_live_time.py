"""Time of the optimizer's grid update with and without live bricks: ``esr_adam_step`` + ``zero_()`` of the gradient (the
dense path: 28 + 4 B per parameter) against ``esr_adam_step_live`` with ``zero_grad=1`` (4 B per parameter, 40 B more on
the live share f: 24 read, 12 written, 4 to zero the gradient) on the SAME buffers in the same run.

    python tools/adam_live_time.py [--sizes c2,g256] [--fractions 0.05,0.25,0.5,1.0] [--repeats 5] [--out profiles/adam_live_time.json]

Workload: one synthetic flat parameter set of C2's size (54.6 M values) and one of the 256^3 size (13 * 256^3 = 218 M: sdf
+ two six-channel colour grids) with its gradient and both moments.  A share f of the bricks is live AND has a gradient, in
contiguous runs of 12 bricks -- a z-column of a channels-last colour grid at 256 nodes is 1536 values -- placed at random;
the rest has zero gradient and zero moments.  Event-timed, median of ``--repeats`` after a warm-up, one process; the
gradient is refilled before every timed call (outside the events), since both paths leave it zero.  Reports the achieved
bytes per second of both paths against their byte models and against a plain copy of the parameter buffer on the same
device, and fails unless the live call is faster than the dense path wherever its byte model is at most half of the
dense path's (f <= 0.3).  One JSON line.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"c2": 54_600_000, "g256": 13 * 256 ** 3}
RUN = 12                      # bricks per contiguous live run
LR, B1, B2, EPS = 0.1, 0.9, 0.99, 1e-8


def timed(fn, prepare, repeats, warmup=2):
    """median milliseconds of fn() by device events; prepare() runs before each call, outside the events"""
    ms = []
    for i in range(warmup + repeats):
        prepare()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="c2,g256")
    ap.add_argument("--fractions", default="0.05,0.25,0.5,1.0")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adam_live_time.py measures on the GPU; none is visible")
    from esr_nerf_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    brick = L.esr_brick_floats()
    out = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, run_bricks=RUN, brick_floats=brick,
               dense_model_bytes_per_param=32, live_model_bytes_per_param="4 + 40 f", sizes={})
    gen = torch.Generator(device=dev).manual_seed(0)
    for size in a.sizes.split(","):
        n = SIZES[size]
        nb = -(-n // brick)
        p = torch.randn(n, device=dev, generator=gen)
        g, g_src, m, v = (torch.empty(n, device=dev) for _ in range(4))
        live = torch.empty(nb, dtype=torch.uint8, device=dev)
        stream = _lib.stream_ptr(dev)
        step = [0]

        def dense():
            step[0] += 1
            _lib.check(L.esr_adam_step(_lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), None, C.c_int64(n), C.c_float(LR),
                                       C.c_float(B1), C.c_float(B2), C.c_float(EPS), C.c_float(0.0), step[0], stream),
                       "esr_adam_step")

        def dense_and_zero():
            dense()
            g.zero_()

        def live_step():
            step[0] += 1
            _lib.check(L.esr_adam_step_live(_lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), None, _lib.ptr(live), n, LR,
                                            B1, B2, EPS, step[0], 1, None, stream), "esr_adam_step_live")

        refill = lambda: g.copy_(g_src)
        spare = torch.empty_like(p)
        copy_ms = timed(lambda: spare.copy_(p), lambda: None, a.repeats)
        del spare
        res = dict(parameters=n, bricks=nb, copy_ms=round(copy_ms, 4), copy_tb_per_s=round(8 * n / copy_ms / 1e9, 3),
                   zero_ms=round(timed(lambda: g.zero_(), lambda: None, a.repeats), 4), fractions={})
        for f in (float(x) for x in a.fractions.split(",")):
            runs = torch.rand(-(-nb // RUN), device=dev, generator=gen) < f
            mask = runs.repeat_interleave(RUN)[:nb]
            if f >= 1.0:
                mask[:] = True
            elem = mask.repeat_interleave(brick)[:n]
            f_real = float(elem.float().mean())
            g_src.normal_(generator=gen).mul_(elem)
            m.normal_(generator=gen).mul_(elem).mul_(0.1)
            v.normal_(generator=gen).abs_().mul_(elem).mul_(0.01)
            live.copy_(mask)
            del elem
            step[0] = 100
            adam_ms = timed(dense, refill, a.repeats)
            dense_ms = timed(dense_and_zero, refill, a.repeats)
            live_ms = timed(live_step, refill, a.repeats)
            torch.cuda.synchronize()
            assert int(torch.count_nonzero(g)) == 0 and int(live.sum()) == int(mask.sum())
            model = 4 + 40 * f_real + 1.0 / brick
            e = dict(live_fraction=round(f_real, 4), adam_ms=round(adam_ms, 4), dense_ms=round(dense_ms, 4), live_ms=round(live_ms, 4),
                     ratio=round(live_ms / dense_ms, 3), model_ratio=round(model / 32, 3),
                     dense_tb_per_s=round(32 * n / dense_ms / 1e9, 3), live_tb_per_s=round(model * n / live_ms / 1e9, 3))
            e["dense_of_copy"] = round(e["dense_tb_per_s"] / res["copy_tb_per_s"], 3)
            e["live_of_copy"] = round(e["live_tb_per_s"] / res["copy_tb_per_s"], 3)
            res["fractions"][str(f)] = e
            print(size, f, json.dumps(e), flush=True)
        out["sizes"][size] = res
        del p, g, g_src, m, v, live
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    slow = [(s, f, e["live_ms"], e["dense_ms"]) for s, r in out["sizes"].items() for f, e in r["fractions"].items()
            if e["model_ratio"] <= 0.5 and not e["live_ms"] < e["dense_ms"]]
    assert not slow, f"the live call is not faster than esr_adam_step + zero_() where its byte model is at most half: {slow}"


if __name__ == "__main__":
    main()
