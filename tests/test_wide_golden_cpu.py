"""The reference pin of the wide conv encoder (tests/golden/encoder_wide_h3.npz: the reference's own ConvEncoder at
model.depth=77 on 2 frames, tests/wide_golden_io.py) against the plain-torch restatement on the CPU.

The float32 restatement runs the reference's arithmetic and must sit inside every bound. The float64 restatement is
exact arithmetic: outputs and gradient norms inside the bounds; sampled elements too, except that the reference's own
f32 gradient of the second stage's conv weight (231 x 154 x 5 x 5, sums over 2 x 32 x 32 pixels) sits 1.08 of the
element bound from float64. The GPU test therefore accepts, per tensor and on the same bounds, the reference's f32
gradient or the float64 one, as test_gpu_dreamer.test_cal_grad_matches_reference does; here the float64 restatement
is held to twice the element bound, and the figures are printed."""
import numpy as np
import torch

import wide_golden_io as wg


def test_fixture_is_small_and_complete():
    z = np.load(wg.FIXTURE)
    assert z["out"].shape == (wg.FRAMES, 4928) and wg.WIDTHS == (154, 231, 308, 308)
    assert sorted(z.files) == sorted(["out", "loss"] + [f"g_{k}__{s}" for k in wg.shapes() for s in ("n", "s")])
    assert sum(z[f"g_{k}__s"].size for k in wg.shapes()) == 12 * 32
    f = wg.frames()
    assert f.shape == (2, 1, 64, 64, 3) and 0.0 <= f.min() and f.max() < 1.0 and not np.array_equal(f[0], f[1])


def test_restatements_match_the_reference():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    z = np.load(wg.FIXTURE)
    out32, g32 = wg.restate(torch.float32)
    do, per = wg.distance(out32, g32, z)
    print("float32 restatement: output", do, "worst gradient", wg.worst(per))
    assert do <= 1.0 and wg.worst(per)[0] <= 1.0
    assert abs(float((out32 * wg.probe()).sum()) - float(z["loss"])) <= 1e-4 * abs(float(z["loss"]))
    out64, g64 = wg.restate(torch.float64)
    do, per = wg.distance(out64, g64, z)
    print("float64 restatement: output", do, {k[len(wg.PREFIX):]: tuple(round(x, 3) for x in v) for k, v in per.items()})
    assert do <= 1.0 and max(v[0] for v in per.values()) <= 1.0
    assert max(v[1] for v in per.values()) <= 2.0
    assert [k for k, v in per.items() if v[1] > 1.0] in ([], [wg.PREFIX + "layers.4.weight"])
