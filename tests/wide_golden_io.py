"""The reference pin of the wide conv encoder (tests/golden/encoder_wide_h3.npz, written by
tests/golden/gen_golden_wide.py): the reference's own ConvEncoder at model.depth=77 (its h3_wider_cnn control:
stages 154 / 231 / 308 / 308, out_dim 4928) on 2 frames. Parameters, frames and the probe of the loss come from the
seeded formulas below, shared by the generator and the tests: no weights are stored. Test infrastructure.

The fixture holds the 2 x 4928 outputs and, under the probe loss sum(out * probe), every parameter gradient's L2 norm
and 32 sampled elements (golden_io.sample_idx) in the reference's names and layouts.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from golden_io import sample_idx
from oracle.init import params_for

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "encoder_wide_h3.npz")
DEPTH, MULTS, KS, SEED, FRAMES = 77, (2, 3, 4, 4), 5, 3, 2
WIDTHS = tuple(DEPTH * m for m in MULTS)
PREFIX = "encoder.encoders.0."
EPS = 1e-4
# bounds (test_gpu_imgrad.py / test_cal_grad_matches_reference): gradient norms within 2e-4, sampled elements within
# 2e-3 relative + 1e-4 of the largest sampled |g|; outputs within 1e-4 + 1e-4 |ref| (test_gpu_fullsize.py's states)
NORM_REL, ELEM_REL, ELEM_MAX, OUT_RTOL, OUT_ATOL = 2e-4, 2e-3, 1e-4, 1e-4, 1e-4


def shapes():
    """parameter name (a checkpoint's) -> shape in the reference's layout, in the reference's order"""
    out, ci = {}, 3
    for i, co in enumerate(WIDTHS):
        out[f"{PREFIX}layers.{4 * i}.weight"] = (co, ci, KS, KS)
        out[f"{PREFIX}layers.{4 * i}.bias"] = (co,)
        out[f"{PREFIX}layers.{4 * i + 2}.weight"] = (co,)
        ci = co
    return out


def params():
    return params_for(shapes(), SEED)


def frames():
    """(FRAMES, 1, 64, 64, 3) float32 in [0, 1): smooth structure plus noise, so pooling windows are not all alike"""
    rng = np.random.default_rng([SEED, 77])
    yy, xx = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    base = 0.5 + 0.25 * np.sin(0.2 * yy[None, :, :, None] + np.arange(FRAMES)[:, None, None, None]) * np.cos(
        0.15 * xx[None, :, :, None] + np.arange(3)[None, None, None, :])
    img = np.clip(base + 0.2 * rng.standard_normal((FRAMES, 64, 64, 3)), 0.0, 0.999)
    return img.astype(np.float32)[:, None]


def probe():
    rng = np.random.default_rng([SEED, 78])
    return rng.standard_normal((FRAMES, WIDTHS[-1] * 16)).astype(np.float32)


def restate(dtype=torch.float64):
    """the encoder restated in plain torch (networks.py:192-234) -> (out (FRAMES, 4928), {name: gradient}) in dtype"""
    P = {k: torch.tensor(v, dtype=dtype).requires_grad_(True) for k, v in params().items()}
    x = torch.tensor(frames(), dtype=dtype).reshape(FRAMES, 64, 64, 3) - 0.5
    x = x.permute(0, 3, 1, 2)
    for i in range(len(WIDTHS)):
        w, b = P[f"{PREFIX}layers.{4 * i}.weight"], P[f"{PREFIX}layers.{4 * i}.bias"]
        lo, hi = (KS - 1) // 2, (KS - 1) - (KS - 1) // 2
        x = F.max_pool2d(F.conv2d(F.pad(x, [lo, hi, lo, hi]), w, b), 2, 2)
        x = F.rms_norm(x.permute(0, 2, 3, 1), (x.shape[1],), P[f"{PREFIX}layers.{4 * i + 2}.weight"], EPS)
        x = F.silu(x).permute(0, 3, 1, 2)
    out = x.reshape(FRAMES, -1)
    gr = torch.autograd.grad((out * torch.tensor(probe(), dtype=dtype)).sum(), list(P.values()))
    return out.detach().numpy(), {k: g.numpy() for k, g in zip(P, gr)}


def summarise(out, grads):
    """the fixture's arrays from an output and a {name: gradient (reference layout)} dict"""
    arrs = {"out": np.asarray(out, np.float32)}
    for k, g in grads.items():
        flat = np.asarray(g, np.float64).reshape(-1)
        arrs[f"g_{k}__n"] = np.asarray(np.linalg.norm(flat))
        arrs[f"g_{k}__s"] = flat[sample_idx(k, flat.size)]
    return arrs


def distance(out, grads, z):
    """(fraction of the output bound used, {name: (fraction of the norm bound, of the element bound)}) against the
    arrays z (the fixture, or summarise() of another answer)"""
    ref = np.asarray(z["out"], np.float64)
    do = float((np.abs(np.asarray(out, np.float64) - ref) / (OUT_ATOL + OUT_RTOL * np.abs(ref))).max())
    per = {}
    for k in shapes():
        flat = np.asarray(grads[k], np.float64).reshape(-1)
        rn, rs = float(z[f"g_{k}__n"]), np.asarray(z[f"g_{k}__s"], np.float64)
        dn = abs(float(np.linalg.norm(flat)) - rn) / (NORM_REL * max(rn, 1e-9))
        got = flat[sample_idx(k, flat.size)]
        de = float((np.abs(got - rs) / (ELEM_REL * np.abs(rs) + ELEM_MAX * np.abs(rs).max() + 1e-12)).max())
        per[k] = (dn, de)
    return do, per


def worst(per):
    return max((max(v), k) for k, v in per.items())
