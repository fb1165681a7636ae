"""The split-bf16 direct bwd-weight kernels (csrc/conv.hip, conv_wgrad3_direct<TM, NBW, WS, PL>) on inputs where the
result is exact, so a wrong lane, tap, plane or a misaligned transposed read of the B operand cannot hide in a tolerance.

Inputs: x and dy are 0 or n +- 2^-9 with n a small non-zero integer, so split2's planes are hi = bf16(v) = +-n and
lo = bf16(v - hi) = +-2^-9, both non-zero, and the three products the kernel keeps (hi hi, hi lo, lo hi) are multiples
of 2^-9. The reference is their float64 sum, the planes restated on the CPU. Where, for every output element, the sum
of the absolute terms stays below 2^24 units of 2^-9 (asserted on the reference, also without a GPU:
test_reference_is_exact_in_fp32), every partial sum is an fp32 number in any order, and [dW | db] must EQUAL the
reference.

Shapes (Ci, Co, H, W, k, Nb): the smallest that reach a rung, a block spanning or straddling taps, an even kernel, rows
past Co in the last 16-row tile, R = 1, gx = 2 and the second pass over the row blocks. Each case asserts that the
library's slab query takes the shape on the split-bf16 kernel (and the rung tests/conv_models.py restates), so it
cannot pass on another kernel.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_models as cm

DEV = "cuda"
UNIT = 2.0 ** -9
LIMIT = 2.0 ** 24  # units of UNIT

# (Ci, Co, H, W, k, Nb, pooled, the rung (tm, nbw, gx), the integer magnitudes)
CASES = {
    "pool_c4_co32": (4, 32, 16, 16, 5, 2, True, (2, 7, 1), (1, 2, 3)),   # <2,7,WS,PL>: a block spans four taps
    "pool_c4_co16": (4, 16, 16, 16, 5, 2, True, (1, 7, 1), (1, 2, 3)),   # <1,7,WS,PL>
    "ci24": (24, 32, 8, 8, 5, 2, False, (2, 5, 1), (1, 2, 3)),           # blocks straddle taps
    "k4_h12": (16, 32, 12, 8, 4, 1, False, (2, 4, 1), (1, 2, 3)),        # even kernel, a 12-row block
    "co24": (16, 24, 16, 16, 5, 2, False, (2, 4, 1), (1, 2, 3)),         # rows >= Co of the last 16-row tile
    "tm3_nbw7": (32, 48, 8, 8, 5, 1, False, (3, 7, 1), (1, 2, 3)),
    "tm4_nbw4": (32, 64, 8, 8, 3, 1, False, (4, 4, 1), (1, 2, 3)),
    "tm1_nbw5_gx2": (48, 16, 8, 8, 5, 2, False, (1, 5, 2), (1, 2, 3)),
    "w128_r1": (16, 32, 3, 128, 3, 1, False, (2, 2, 1), (1, 2, 3)),      # one image row per block
    "nb260": (16, 16, 8, 8, 3, 260, False, (1, 2, 1), (1, 2)),           # 260 row blocks over 256 slabs
}
BORDER = "tm3_nbw7"  # pad 2


def _dyadic(shape, mags, g, density=0.5):
    n = torch.tensor(mags, dtype=torch.float32)[torch.randint(0, len(mags), shape, generator=g)]
    sign = 1.0 - 2.0 * torch.randint(0, 2, shape, generator=g)
    lo = UNIT * (1.0 - 2.0 * torch.randint(0, 2, shape, generator=g))
    keep = torch.rand(shape, generator=g) < density
    return torch.where(keep, sign * n + lo, torch.zeros(shape))


def _split(v):
    """split2 restated: hi = bf16(v), lo = bf16(v - hi), as float64"""
    hi = v.to(torch.bfloat16).float()
    lo = (v - hi).to(torch.bfloat16).float()
    return hi.double(), lo.double()


def _wgrad64(x, dy, k):
    """[dW as (ky, kx, ci) | db] (Co, k k Ci + 1) in the tensors' dtype; pads as oracle/ref_cpu.conv_same"""
    Nb, H, W, Ci = x.shape
    lo, hi = (k - 1) // 2, (k - 1) - (k - 1) // 2
    xp = F.pad(x, [0, 0, lo, hi, lo, hi])
    cols = [torch.einsum("nhwo,nhwc->oc", dy, xp[:, ky:ky + H, kx:kx + W, :]) for ky in range(k) for kx in range(k)]
    return torch.cat(cols + [dy.sum((0, 1, 2))[:, None]], 1)


@functools.lru_cache(maxsize=None)
def case_data(name, border=False):
    """x, the kernel's gradient operand (dy, or dpool and amax), the reference and its worst sum of |terms| in units"""
    Ci, Co, H, W, k, Nb, pooled, _, mags = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 1000 * border)
    x = _dyadic((Nb, H, W, Ci), mags, g)
    if border:
        inner = torch.zeros(H, W, dtype=torch.bool)
        inner[1:H - 1, 1:W - 1] = True
        x[:, inner] = 0.0
        assert x.abs().sum() > 0
    if pooled:
        dpool = _dyadic((Nb, H // 2, W // 2, Co), mags, g, density=1.0)
        amax = torch.randint(0, 4, dpool.shape, generator=g).to(torch.uint8)
        win = torch.zeros(Nb, H // 2, W // 2, Co, 4)
        win.scatter_(-1, amax.long()[..., None], dpool[..., None])  # window position 2 dy + dx
        dy = win.reshape(Nb, H // 2, W // 2, Co, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(Nb, H, W, Co)
        grad = (dpool, amax)
    else:
        dy = _dyadic((Nb, H, W, Co), mags, g)
        grad = (dy,)
    (xh, xl), (dh, dl) = _split(x), _split(dy)
    assert torch.equal(xh + xl, x.double()) and torch.equal(dh + dl, dy.double()), "hi + lo is the value"
    assert (xl != 0).sum() == (x != 0).sum() > 0 and (dl != 0).sum() == (dy != 0).sum() > 0, "both planes are used"
    ref = _wgrad64(xh, dh + dl, k) + _wgrad64(xl, dh, k)  # hi hi + hi lo + lo hi; the bias column's x is (1, 0)
    ref[:, -1] = (dh + dl).sum((0, 1, 2))
    mag = _wgrad64(xh.abs(), dh.abs() + dl.abs(), k) + _wgrad64(xl.abs(), dh.abs(), k)
    mag[:, -1] = (dh.abs() + dl.abs()).sum((0, 1, 2))
    return x, grad, ref.numpy(), float(mag.max()) / UNIT


def _assert_exact_condition(name, border=False):
    _, _, ref, units = case_data(name, border)
    assert units < LIMIT, f"{name}: sum of |terms| reaches {units:.3g} units of 2^-9 (limit 2^24)"
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), "the reference is an fp32 array"
    assert np.abs(ref).max() > 0


@pytest.mark.parametrize("name", list(CASES))
def test_reference_is_exact_in_fp32(name):
    _assert_exact_condition(name)
    if name == BORDER:
        _assert_exact_condition(name, True)


def _assert_rung(name):
    """the library's own plan takes the shape on the split-bf16 kernel, at the rung the case names"""
    from sdreamer import _native as nat, kernels as K
    Ci, Co, H, W, k, Nb, pooled, (tm, nbw, gx), _ = CASES[name]
    assert K.FAST_GEMM and K.WGRAD1_X3, "the default switches"
    if pooled:
        pl = cm.pool3_plan(Nb, H, W, Ci, Co, k, k)
        got = nat.fns["sd_conv2d_wgrad_pool_bf16x3_slabs"](Nb, H, W, Ci, Co, k, k)
    else:
        pl = cm.direct3_plan(Nb, H, W, Ci, Co, k, k)
        got = nat.fns["sd_conv2d_wgrad_bf16x3_slabs"](Nb, H, W, Ci, Co, k, k, 0)
    assert pl and (pl["tm"], pl["nbw"], pl["gx"], pl["ws"]) == (tm, nbw, gx, pooled), (name, pl)
    assert got == pl["slabs"] > 0, (name, got, pl)
    if name == "nb260":
        assert Nb * (H // pl["R"]) > pl["slabs"], "more row blocks than slabs"
    if name == "w128_r1":
        assert pl["R"] == 1


def _run(name, border=False):
    from sdreamer import kernels as K
    _assert_rung(name)
    _assert_exact_condition(name, border)
    k = CASES[name][4]
    x, grad, ref, units = case_data(name, border)
    if len(grad) == 2:
        got = K.conv2d_wgrad_pool(x.to(DEV), grad[0].to(DEV), grad[1].to(DEV), k, k)
    else:
        got = K.conv2d_wgrad(x.to(DEV), grad[0].to(DEV), k, k, fast=True)
    got = got.double().cpu().numpy()
    assert got.shape == ref.shape
    bad = np.argwhere(got != ref)
    print(f"{name}{' border' if border else ''}: {len(bad)} of {ref.size} elements differ, "
          f"max |diff| {np.abs(got - ref).max():.3g}, sum |terms| {units:.3g} units")
    assert len(bad) == 0, (f"{name}: {len(bad)} of {ref.size} elements differ from the exact reference, first "
                           f"(co, j) = {tuple(bad[0])}: {got[tuple(bad[0])]!r} vs {ref[tuple(bad[0])]!r}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_wgrad3_exact(name):
    _run(name)


@pytest.mark.gpu
def test_wgrad3_exact_border_pixels():
    """the only non-zero input pixels lie on the image border (pad 2): what the taps read beyond it is the zero halo"""
    _run(BORDER, border=True)
