"""bench.py --dump-outputs: what the last timed step returned, within 64 MB, sampled the same way in every run (CPU tensors
stand in for the device ones: the helpers only index and copy)."""
import numpy as np
import torch

import bench                    # (the repository root is on sys.path: conftest.py)


def _c2_like():
    g = torch.Generator().manual_seed(0)
    grads = {"sdf.grid": torch.randn(1, 1, 256, 256, 64, generator=g),
             # the colour grids' gradients are permuted views of a channels-last buffer (trainer.FineStep)
             "off_color.grid": torch.randn(1, 256, 256, 64, 6, generator=g).permute(0, 4, 1, 2, 3),
             "emo_color.grid": torch.randn(1, 256, 256, 64, 6, generator=g).permute(0, 4, 1, 2, 3),
             "off_rgbnet.linear.0.weight": torch.randn(192, 85, generator=g)}
    outs = {"etc/emit": torch.randn(1000, 3, dtype=torch.float64, generator=g), "cnt": torch.arange(10)}
    return torch.tensor([0.25]), grads, outs


def test_dump_is_bounded_and_deterministic():
    res = _c2_like()
    arrays = bench.dump_arrays(res)
    assert set(arrays) == {"loss", "grad.sdf.grid", "grad.off_color.grid", "grad.emo_color.grid",
                           "grad.off_rgbnet.linear.0.weight", "out.etc.emit", "out.cnt"}
    a, b = bench.dump_sample(arrays), bench.dump_sample(bench.dump_arrays(res))
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BYTES < 64 * 10**6
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    # small arrays whole and exact, in their own shape; integers and float64 as float64
    assert np.array_equal(a["loss"], res[0].numpy()) and np.array_equal(a["grad.sdf.grid"], res[1]["sdf.grid"].numpy())
    assert a["out.etc.emit"].dtype == np.float64 and np.array_equal(a["out.cnt"], np.arange(10, dtype=np.float64))
    assert 0 < a["grad.off_color.grid"].size < res[1]["off_color.grid"].numel()
    assert not np.array_equal(a["grad.off_color.grid"], a["grad.emo_color.grid"])      # another name, another sample


def test_cut_array_holds_the_seeded_elements_in_row_major_order():
    t = _c2_like()[1]["off_color.grid"]                    # a permuted (non-contiguous) view
    s = bench.dump_sample({"grad.off_color.grid": t}, budget=4000)["grad.off_color.grid"]
    idx = bench.dump_index("grad.off_color.grid", t.numel(), 1000)
    assert 0 < len(idx) <= 1000 and np.array_equal(s, t.contiguous().reshape(-1).numpy()[idx])

