"""The resampling patch compositor (sd_patch_apply_affine / sd_patch_grad_affine, include/sdhip.h) restated in torch on
the CPU: the reference (float64) and the restatement (float32) of the kernels' arithmetic, differentiable in the patch
by autograd, with planted faults, the derived error bounds and the case table. Test infrastructure, not a test.

Per pixel (y, x) of image n with the row a00 a01 b0 a10 a11 b1 gain bias: u = a00 y + a01 x + b0, v = a10 y + a11 x + b1,
i0 = floor(u), j0 = floor(v), fu = u - i0, fv = v - j0; the taps (i0 + di, j0 + dj) weigh (1 - fu | fu)(1 - fv | fv),
those outside the patch contribute nothing; alpha = the sum of the in-range weights, q = the same sum over
P(patch[tap]) with P(p) = clamp(gain (p - 0.5) + 0.5 + bias, 0, 1); out = q + (1 - alpha) in.

Bounds (derived, not measured; 2^-24 is the unit roundoff of f32):
  delta_n = 4 * 2^-24 * max(|a00| (H - 1) + |a01| (W - 1) + |b0|, |a10| (H - 1) + |a11| (W - 1) + |b1|) bounds the f32 error
    of a coordinate of image n (two products, two sums, each relative to a partial sum no larger than that maximum);
    the reference reads the same f32-rounded rows, promoted, so the rows themselves carry no error.
  forward: |got - ref| <= 4 delta_n + 4 * 2^-23 per element: q + (1 - alpha) in is a bilinear interpolant of values in
    [0, 1] (the patch's P, or the input where the mask is zero): 2-Lipschitz in each coordinate, two coordinates, and
    continuous across tap and border changes; the second term covers the roundings of the weights, P, the sums, the
    blend and in = byte / 255. Clamp kinks are kept out by the margin condition (MARGIN).
  gradient: |got - ref|_e <= 2 delta_max C_e + (n_e + 8) 2^-24 S_e with C_e = sum |gain dimg| over the element's support
    pixels (a weight is 1-Lipschitz in each coordinate), S_e = sum w |gain dimg| and n_e the number of support pixels
    (one rounding per accumulation, a few per term).
"""
import math

import torch

H, W, C, CP, PH, PW, NB = 12, 20, 3, 4, 5, 7, 33
CHUNK = 32  # SD_PATCH_CHUNK: NB = 33 gives two chunks, the second with one image
MARGIN = 1e-3  # every case: |gain (p - 0.5) + 0.5 + bias - {0, 1}| >= MARGIN for every image and patch element
FAULTS = ("swap_fractions", "row_tap_off_by_one", "no_clamp_derivative", "skip_chunk_boundary")
U = 2.0 ** -24


def _coords(tf, dtype):
    """u, v (N, H, W) in `dtype` from the f32 rows promoted (the kernel's association: a00 y + (a01 x + b0))"""
    t = tf.to(dtype)
    y = torch.arange(H, dtype=dtype).view(1, H, 1)
    x = torch.arange(W, dtype=dtype).view(1, 1, W)
    r = lambda k: t[:, k].view(-1, 1, 1)  # noqa: E731
    return r(0) * y + (r(1) * x + r(2)), r(3) * y + (r(4) * x + r(5))


def photometric(patch, tf, dtype, fault=None):
    """P_n(patch): (N, ph, pw, C)"""
    t = tf.to(dtype)
    gain, bias = t[:, 6].view(-1, 1, 1, 1), t[:, 7].view(-1, 1, 1, 1)
    lin = gain * (patch.to(dtype).unsqueeze(0) - 0.5) + 0.5 + bias
    out = lin.clamp(0.0, 1.0)
    if fault == "no_clamp_derivative":  # the clamp's value with the derivative of the line
        out = out.detach() + (lin - lin.detach())
    return out, lin


def composite(images, patch, tf, dtype=torch.float64, fault=None):
    """images (N, H, W, C) in [0, 1] (any float dtype), patch (ph, pw, C), tf (N, 8) f32 -> the composited images in
    `dtype`, differentiable in the patch"""
    assert fault in (None,) + FAULTS
    N = images.shape[0]
    u, v = _coords(tf, dtype)
    i0, j0 = torch.floor(u), torch.floor(v)
    fu, fv = u - i0, v - j0
    if fault == "swap_fractions":
        fu, fv = fv, fu
    P, _ = photometric(patch, tf, dtype, fault)
    n_idx = torch.arange(N).view(N, 1, 1).expand(N, H, W)
    q = torch.zeros(N, H, W, C, dtype=dtype)
    alpha = torch.zeros(N, H, W, dtype=dtype)
    for di in (0, 1):
        for dj in (0, 1):
            i = i0 + (di if not (fault == "row_tap_off_by_one" and di) else 2)
            j = j0 + dj
            ok = (i >= 0) & (i < PH) & (j >= 0) & (j < PW)
            w = ((fu if di else 1 - fu) * (fv if dj else 1 - fv)) * ok.to(dtype)
            tap = P[n_idx, i.clamp(0, PH - 1).long(), j.clamp(0, PW - 1).long()]
            q = q + w.unsqueeze(-1) * tap
            alpha = alpha + w
    return q + (1 - alpha).unsqueeze(-1) * images.to(dtype)


def gradient(images, patch, tf, dimg, dtype=torch.float64, fault=None):
    """d <composite, dimg> / d patch (ph, pw, C) by autograd, in `dtype`"""
    p = patch.to(dtype).clone().requires_grad_(True)
    g = dimg.to(dtype).clone()
    if fault == "skip_chunk_boundary":  # the image at which the second chunk starts is left out of the sum
        g[CHUNK] = 0.0
    (composite(images, p, tf, dtype, fault) * g).sum().backward()
    return p.grad


def hat_weights(tf, widen=0.0):
    """float64 W (N, H, W, ph, pw): the bilinear weight of patch element (i, j) at pixel (y, x) as
    hat(u - i) hat(v - j), hat(t) = max(0, 1 - |t|) (the tap formulation's weights, zero padding included), and the
    support mask |u - i| < 1 + widen, |v - j| < 1 + widen"""
    u, v = _coords(tf, torch.float64)
    du = (u.unsqueeze(-1) - torch.arange(PH, dtype=torch.float64)).abs()  # (N, H, W, ph)
    dv = (v.unsqueeze(-1) - torch.arange(PW, dtype=torch.float64)).abs()
    w = (1 - du).clamp_min(0).unsqueeze(-1) * (1 - dv).clamp_min(0).unsqueeze(-2)
    wd = widen.view(-1, 1, 1, 1) if torch.is_tensor(widen) else widen
    supp = (du < 1 + wd).unsqueeze(-1) & (dv < 1 + wd).unsqueeze(-2)
    return w, supp


def delta(tf):
    """(N,) float64: the worst f32 error of a coordinate per image"""
    a = tf.double().abs()
    return 4 * U * torch.maximum(a[:, 0] * (H - 1) + a[:, 1] * (W - 1) + a[:, 2],
                                 a[:, 3] * (H - 1) + a[:, 4] * (W - 1) + a[:, 5])


def forward_bound(tf):
    """(N, 1, 1, 1) float64"""
    return (4 * delta(tf) + 4 * 2.0 ** -23).view(-1, 1, 1, 1)


def gradient_bound(tf, dimg):
    """(ph, pw, C) float64"""
    d = delta(tf)
    w, supp = hat_weights(tf, widen=d)
    g = (tf[:, 6].double().view(-1, 1, 1, 1) * dimg.double()).abs()  # (N, H, W, C)
    c_e = torch.einsum("nyxij,nyxc->ijc", supp.double(), g)
    s_e = torch.einsum("nyxij,nyxc->ijc", w, g)
    n_e = supp.sum(dim=(0, 1, 2)).double().unsqueeze(-1)
    return 2 * float(d.max()) * c_e + (n_e + 8) * U * s_e


def margin(patch, tf):
    """the smallest distance of gain (p - 0.5) + 0.5 + bias from 0 and 1 over the images and patch elements"""
    _, lin = photometric(patch, tf, torch.float64)
    return float(torch.minimum(lin.abs(), (lin - 1).abs()).min())


# ------------------------------------------------------------------------------------------------- the case table
def rows(offsets, scale, theta, gain=1.0, bias=0.0):
    """sdreamer.attack.transform_rows on per-image lists / scalars"""
    from sdreamer.attack import transform_rows
    n = len(offsets)
    col = lambda v: torch.as_tensor(v, dtype=torch.float64).expand(n) if not torch.is_tensor(v) else v.double()  # noqa: E731
    return transform_rows(torch.tensor(offsets), torch.stack([col(scale), col(theta), col(gain), col(bias)], 1),
                          (PH, PW))


def inputs(seed=0):
    """the shared inputs: uint8 and f32 images, the patch (values (k + 0.5) / 67: every case keeps MARGIN from the
    clamp's kinks, and gain 1.3 / bias -0.1 clamps the largest and the smallest of them), d_image"""
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (NB, H, W, C), generator=g, dtype=torch.uint8)
    f32 = torch.rand(NB, H, W, C, generator=g)
    k = torch.cat([torch.randperm(67, generator=g), torch.randperm(67, generator=g)])[:PH * PW * C]
    patch = ((k.double() + 0.5) / 67).to(torch.float32).view(PH, PW, C)
    dimg = torch.randn(NB, H, W, C, generator=g)
    return dict(u8=u8, f32=f32, patch=patch, dimg=dimg)


def case_table(seed=1):
    """name -> tf (NB, 8) f32"""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda lo, hi: lo + (hi - lo) * torch.rand(NB, generator=g, dtype=torch.float64)  # noqa: E731
    inside = [[int(torch.randint(0, H - PH + 1, (1,), generator=g)), int(torch.randint(0, W - PW + 1, (1,), generator=g))]
              for _ in range(NB)]
    mixed = [[int(torch.randint(-PH - 1, H + 2, (1,), generator=g)), int(torch.randint(-PW - 1, W + 2, (1,), generator=g))]
             for _ in range(NB)]
    mixed[:4] = [[-2, -3], [H - 2, W - 3], [3, 5], [-PH, 4]]  # over a corner, over the other, inside, just outside
    cases = {"identity": rows(mixed, 1.0, 0.0)}
    sub = rows(inside, 1.0, 0.0)
    sub[:, 2] -= rnd(0.0, 1.0).float()
    sub[:, 5] -= rnd(0.0, 1.0).float()
    cases["subpixel"] = sub
    r90 = rows(mixed, 1.0, math.pi / 2)
    r90[r90.abs() < 1e-6] = 0.0  # cos(pi / 2) in float64 is 6e-17: exactly 90 degrees
    cases["rot90"] = r90
    cases["rotation"] = rows(inside, 1.0, rnd(-35.0, 35.0) * math.pi / 180)
    cases["scale"] = rows(inside, rnd(0.75, 1.25), 0.0)
    # scale 2: the 10 x 14 window centred on the bottom edge, the right edge, or the top-left corner
    half = [[[H - 1 - PH // 2, 6], [4, W - 1 - PW // 2], [-(PH // 2), -(PW // 2)]][n % 3] for n in range(NB)]
    cases["scale2_half_off"] = rows(half, 2.0, rnd(-0.2, 0.2))
    away = [[[-40, -40], [100, 3], [2, 100]][n % 3] for n in range(NB)]
    cases["off_image"] = rows(away, rnd(0.75, 1.25), rnd(-0.6, 0.6))
    cases["photometric"] = rows(inside, rnd(0.9, 1.1), rnd(-10.0, 10.0) * math.pi / 180, 1.3, -0.1)
    return cases


def plain_offsets(tf):
    """the int32 offsets (N, 2) of identity rows"""
    return torch.stack([-tf[:, 2], -tf[:, 5]], 1).round().to(torch.int32)
