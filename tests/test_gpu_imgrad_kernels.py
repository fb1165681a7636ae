"""The first encoder stage's input gradient: sd_conv2d_dgrad_pool (the pooled gradient + argmax expanded in LDS), the
fallback for shapes it refuses, and the two stage Functions' input-gradient branch for a channel-padded input."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-4


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _expand(dpool, amax):
    """(Nb, Ho, Wo, C) pooled gradient + argmax (q = 2 * dy + dx) -> (Nb, 2 Ho, 2 Wo, C), zeros off the argmax"""
    Nb, Ho, Wo, C = dpool.shape
    out = torch.zeros(Nb, Ho, 2, Wo, 2, C, dtype=dpool.dtype)
    for q in range(4):
        out[:, :, q >> 1, :, q & 1, :] = torch.where(amax == q, dpool, torch.zeros_like(dpool))
    return out.reshape(Nb, 2 * Ho, 2 * Wo, C)


def _dgrad64(dconv, w):
    """float64 input gradient of the same-padded stride-1 conv: dconv (Nb, H, W, Co), w (Co, kh, kw, Ci) -> NHWC"""
    wk = w.double().permute(0, 3, 1, 2)  # (Co, Ci, kh, kw)
    pad = (w.shape[1] - 1) // 2
    return F.conv_transpose2d(dconv.double().permute(0, 3, 1, 2), wk, padding=pad).permute(0, 2, 3, 1)


@pytest.mark.parametrize("nb,h", [(3, 64), (2, 40), (2, 2)])
def test_dgrad_pool_planned_shape(nb, h):
    """conv2d_dgrad_pool at the planned shape (Co 32, Ci 3, 5x5, W 64; H = 64, a height that is no multiple of the
    16-row tile, and the smallest one) against float64 conv_transpose2d of the expanded gradient. The argmax takes all
    four window positions in every pooled pixel (so at every border and corner), one image's gradient is all zero
    (its result must be exactly zero). Bound per element 2e-5 * sum |dconv| |w| over its taps in float64: the
    library's ~1e-5 of sum |a b| for its split-bf16 contractions, doubled for the reorder; this kernel is plain f32
    FMA and sits far inside (measured worst ratio printed)."""
    from sdreamer import kernels as K
    co, ci, wd = 32, 3, 64
    ho, wo = h // 2, wd // 2
    dpool = torch.randn(nb, ho, wo, co, generator=_g(1))
    dpool[nb // 2] = 0.0
    yo, xo, c, n = torch.meshgrid(torch.arange(ho), torch.arange(wo), torch.arange(co), torch.arange(nb),
                                  indexing="ij")
    amax = ((7 * yo + 3 * xo + c + n) % 4).permute(3, 0, 1, 2).contiguous().to(torch.uint8)
    for q in range(4):  # every position at every pooled pixel, so at each border and corner
        assert bool((amax == q).any(-1).all())
    w = torch.randn(co, 5, 5, ci, generator=_g(2)) / (ci * 25) ** 0.5
    before = K.DGRAD_POOL_CALLS
    got = K.conv2d_dgrad_pool(dpool.to(DEV), amax.to(DEV), w.to(DEV))
    assert got is not None and got.shape == (nb, h, wd, ci)
    assert K.DGRAD_POOL_CALLS == before + 1
    dconv = _expand(dpool, amax)
    ref = _dgrad64(dconv, w)
    bound = 2e-5 * _dgrad64(dconv.abs(), w.abs())
    err = (got.cpu().double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300))[bound > 0].max())
    print(f"conv2d_dgrad_pool nb={nb} h={h}: worst |err| / bound = {ratio:.4f}")
    assert float((err - bound).max()) <= 0, ratio
    assert torch.equal(got[nb // 2].cpu(), torch.zeros(h, wd, ci))
    again = K.conv2d_dgrad_pool(dpool.to(DEV), amax.to(DEV), w.to(DEV))
    assert torch.equal(got, again)


def test_dgrad_pool_refuses_other_shapes():
    from sdreamer import kernels as K
    for ho, wo, co, ci, ks in [(16, 16, 16, 3, 5), (32, 32, 32, 4, 5), (32, 32, 32, 3, 3), (32, 16, 32, 3, 5)]:
        dpool = torch.zeros(1, ho, wo, co, device=DEV)
        amax = torch.zeros(1, ho, wo, co, dtype=torch.uint8, device=DEV)
        assert K.conv2d_dgrad_pool(dpool, amax, torch.zeros(co, ks, ks, ci, device=DEV)) is None


def _stage64(x, w, b, nw, gy):
    """float64 conv -> max_pool2d -> rms2d -> silu under autograd; x (Nb, H, W, Ci) NHWC already shifted. Returns
    (y NHWC, dx NHWC, sum |dconv| |w| per input element, the smallest top-two gap of the pooling windows)."""
    x = x.double().requires_grad_()
    wk = w.double().permute(0, 3, 1, 2)
    conv = F.conv2d(x.permute(0, 3, 1, 2), wk, b.double(), padding=(w.shape[1] - 1) // 2)
    conv.retain_grad()
    pooled = F.max_pool2d(conv, 2)
    y = F.silu(pooled * torch.rsqrt((pooled * pooled).mean(1, keepdim=True) + EPS) * nw.double()[None, :, None, None])
    y.backward(gy.double().permute(0, 3, 1, 2))
    Nb, Co, H, W = conv.shape
    win = conv.detach().reshape(Nb, Co, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(Nb, Co, H // 2, W // 2, 4)
    top = win.topk(2, -1).values
    mag = F.conv_transpose2d(conv.grad.abs(), wk.abs(), padding=(w.shape[1] - 1) // 2).permute(0, 2, 3, 1)
    return y.detach().permute(0, 2, 3, 1), x.grad, mag, float((top[..., 0] - top[..., 1]).min())


@pytest.mark.parametrize("hw,co,ci,raw", [(32, 16, 3, False), (32, 16, 3, True), (32, 16, 1, False), (32, 16, 1, True),
                                          (64, 32, 3, False), (64, 32, 3, True)])
def test_stage_input_gradient_matches_float64(hw, co, ci, raw):
    """ConvPoolNormFn forward, then backward to a channel-padded input, against float64 conv -> max_pool2d -> rms2d
    -> silu under autograd: 32x32 / Co 16 with Ci 3 and Ci 1 (refused by the kernel: sd_pool_rms_bwd + the dgrad on
    the zero-padded weight) and the planned shape (the pooled-gradient kernel). raw: the image itself is the input
    (the stage shifts and pads it, the gradient has the image's channels); else x carries the pad channels and their
    gradient must be zero. Bound per element 4e-5 * sum |dconv| |w| (float64) + 1e-7 * max |ref|: 2e-5 for the
    contraction as in test_dgrad_pool_planned_shape, as much again for the f32 forward / pooling backward that formed
    dconv (each a few 1e-7 relative). The pooling windows' smallest top-two gap is asserted large enough that f32 and
    float64 pick the same argmax."""
    from sdreamer import kernels as K
    from sdreamer import ops
    nb, cp = 2, (ci + 3) // 4 * 4
    img = torch.rand(nb, hw, hw, ci, generator=_g(3))
    w = torch.randn(co, 5, 5, ci, generator=_g(4)) / (ci * 25) ** 0.5
    b = 0.1 * torch.randn(co, generator=_g(5))
    nw = 1 + 0.1 * torch.randn(co, generator=_g(6))
    gy = torch.randn(nb, hw // 2, hw // 2, co, generator=_g(7))
    yref, dref, mag, gap = _stage64(img - 0.5, w, b, nw, gy)
    assert gap > 1e-6, gap
    wd, bd, nwd = (t.to(DEV).requires_grad_() for t in (w, b, nw))
    before = K.DGRAD_POOL_CALLS
    if raw:
        x = img.to(DEV).requires_grad_()
        y = ops.ConvPoolNormFn.apply(x, wd, bd, nwd, False, 0.5)
    else:
        x = K.pad_channels(img.to(DEV), cp, 0.5).requires_grad_()
        y = ops.ConvPoolNormFn.apply(x, wd, bd, nwd, False)
    y.backward(gy.to(DEV))
    assert K.DGRAD_POOL_CALLS == before + (1 if (hw, co, ci) == (64, 32, 3) else 0)
    assert float((y.detach().cpu().double() - yref).abs().max()) < 1e-4
    dx = x.grad.cpu().double()
    assert dx.shape[-1] == (ci if raw else cp)
    if not raw:
        assert torch.equal(dx[..., ci:], torch.zeros_like(dx[..., ci:]))
    err = (dx[..., :ci] - dref).abs()
    bound = 4e-5 * mag + 1e-7 * float(dref.abs().max())
    print(f"stage dx hw={hw} co={co} ci={ci} raw={raw}: worst |err| / bound = {float((err / bound).max()):.4f}, "
          f"argmax gap {gap:.2e}")
    assert float((err - bound).max()) <= 0, float((err / bound).max())
    if (hw, co, ci) == (64, 32, 3):
        # the planned shape keeps the compact weight-gradient path: the parameter gradients are bit for bit the ones
        # the stage computes when no input gradient is asked for
        w2, b2, nw2 = (t.to(DEV).requires_grad_() for t in (w, b, nw))
        ops.ConvPoolNormFn.apply(K.pad_channels(img.to(DEV), cp, 0.5), w2, b2, nw2, False).backward(gy.to(DEV))
        for a, r, what in ((wd.grad, w2.grad, "dw"), (bd.grad, b2.grad, "db"), (nwd.grad, nw2.grad, "dnw")):
            assert torch.equal(a, r), what


@pytest.mark.parametrize("raw", [True, False])
def test_film_identity_input_gradient_is_bitwise_the_plain_stage(raw):
    """FilmConvPoolNormFn's promise (gamma = 1, beta = 0: every output and gradient equals ConvPoolNormFn's bit for
    bit) extended to the input gradient, on the planned shape (both take sd_conv2d_dgrad_pool)."""
    from sdreamer import kernels as K
    from sdreamer import ops
    nb, hw, co, ci, T = 4, 64, 32, 3, 2
    img = torch.rand(nb, hw, hw, ci, generator=_g(11)).to(DEV)
    w = (torch.randn(co, 5, 5, ci, generator=_g(12)) / (ci * 25) ** 0.5).to(DEV)
    b = (0.1 * torch.randn(co, generator=_g(13))).to(DEV)
    nw = (1 + 0.1 * torch.randn(co, generator=_g(14))).to(DEV)
    gy = torch.randn(nb, hw // 2, hw // 2, co, generator=_g(15)).to(DEV)
    outs = []
    for film in (False, True):
        ps = [t.clone().requires_grad_() for t in (w, b, nw)]
        x = (img.clone() if raw else K.pad_channels(img, 4, 0.5)).requires_grad_()
        tail = (0.5,) if raw else ()
        before = K.DGRAD_POOL_CALLS
        if film:
            gamma = torch.ones(nb // T, co, device=DEV).requires_grad_()
            beta = torch.zeros(nb // T, co, device=DEV).requires_grad_()
            y = ops.FilmConvPoolNormFn.apply(x, *ps, gamma, beta, False, *tail)
        else:
            y = ops.ConvPoolNormFn.apply(x, *ps, False, *tail)
        y.backward(gy)
        assert K.DGRAD_POOL_CALLS == before + 1
        outs.append((y.detach(), x.grad, *[p.grad for p in ps]))
    for a, r, what in zip(outs[1], outs[0], ("y", "dx", "dw", "db", "dnw")):
        assert torch.equal(a, r), what
    assert outs[0][1].shape[-1] == (3 if raw else 4)
