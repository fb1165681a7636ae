"""The conv encoder / decoder stages (ops.ConvPoolNormFn, ops.FilmConvPoolNormFn, ops.UpConvFn + ops.rms_silu) and the
conv entry points of kernels.py against a float64 torch reference, at the smallest shapes that reach each arm of
csrc/conv.hip's dispatch and of the row kernels' in csrc/poolnorm.hip (tests/conv_models.py: the case tables, with the arm each case reaches; the tie margin, the
comparison functions and their discrimination are checked on the CPU by test_conv_parity_cpu.py; DESIGN.md § 2.2 has
the table and the measured figures).

Per stage case: the forward, the saved argmax (equal at every window, none excluded), and .backward(): dx where it is
wanted, dW, db, dnw and the FiLM gradients, with test_gpu_ops.test_conv_pool_norm's tolerances as caps (2e-5 forward,
5e-5 gradients, of max(max |ref|, 1)). Before each backward a NaN-filled tensor of the conv gradient's size is
allocated and freed, so an element of the conv gradient that no kernel writes shows as NaN instead of happening to be
zero. Each case asserts the arm its row names: the Python plans against the library's queries
(sd_conv2d_wgrad_*_slabs, sd_conv2d_dgrad_pool_ok), K.conv2d_fwd_pool returning None or not, and the count of
conv2d_dgrad_pool calls; the kernel inside a gate (conv_fwd16 or the generic tiles, say) is stated by the plans'
restatement, which the sweep in the CPU file ties to the library.

Per kernel case: |err| <= c * contraction(|a|, |b|) + floor elementwise, c = 4e-5 on the split-bf16 arms
(test_conv_backward_bf16x3's) and 8 x the float32 torch restatement's own worst ratio on the f32 arms (the kernels sum
the same products in another order, MFMA accumulating in chunks of 4).

Out of reach of a few-second test: the `es == false` arms (an input of 2 GiB or more).
"""
import numpy as np
import pytest
import torch

import conv_models as cm

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _nan_scratch(shape):
    """allocate and free NaN-filled tensors of this shape: the caching allocator hands the next torch.empty of the size
    one of them"""
    junk = [torch.full(shape, float("nan"), device=DEV) for _ in range(4)]
    torch.cuda.synchronize()
    del junk


def _f64(t):
    return t.detach().double().cpu().numpy()


def _khwc(w):
    return w.permute(0, 2, 3, 1).contiguous().to(DEV)


def _check_arms(c, monkeypatch):
    from sdreamer import _native as nat, kernels as K, ops
    assert K.CONV6 and K.FAST_GEMM and ops.FUSED_POOL and ops.POOL_COMPACT, "the default switches"
    monkeypatch.setattr(K, "WGRAD1_X3", c.x3)
    assert cm.stage_arms(c) == (c.fwd, c.wgrad, c.dgrad), f"{c.name} left its arm: {cm.stage_arms(c)}"
    cm.check_plans(nat, c.nb, c.H, c.W, c.cx, c.co, c.k)


def run_product_stage(c):
    from sdreamer import kernels as K, ops
    x, w, b, nw, gamma, beta, dy = cm.stage_inputs(c)
    wd, bd, nwd = _khwc(w).requires_grad_(), b.to(DEV).requires_grad_(), nw.to(DEV).requires_grad_()
    pad_shift = None
    if c.raw and c.dx:  # the image's gradient is wanted: the stage pads (and un-pads) itself
        xd, pad_shift = x.to(DEV).requires_grad_(), 0.5
    elif c.raw:
        xd = K.pad_channels(x.to(DEV), c.cx, 0.5)
    else:
        xd = x.to(DEV).requires_grad_(c.dx)
    # the forward arm: the fused launch takes the kernel's operands or returns None
    xk = K.pad_channels(x.to(DEV), c.cx, 0.5) if c.raw else x.to(DEV)
    wk = ops._pad_last(wd.detach(), c.cx) if c.raw else wd.detach()
    film = None
    if c.ipc:
        film = (gamma.to(DEV).requires_grad_(), beta.to(DEV).requires_grad_())
    fused = K.conv2d_fwd_pool(xk, wk, bd.detach(), nwd.detach(), nchw_flat=c.nchw,
                              film=None if film is None else tuple(t.detach() for t in film))
    took = "refused" if fused is None else "taken"
    assert (fused is None) == c.fwd.endswith("+ pool_rms"), f"{c.name}: the fused launch was {took}"
    calls = K.DGRAD_POOL_CALLS
    if c.ipc:
        out = ops.FilmConvPoolNormFn.apply(xd, wd, bd, nwd, film[0], film[1], c.nchw, pad_shift)
    else:
        out = ops.ConvPoolNormFn.apply(xd, wd, bd, nwd, c.nchw, pad_shift)
    assert out.shape == dy.shape
    amax = out.grad_fn.saved_tensors[5]
    got = dict(y=_f64(out), amax=amax.cpu().numpy())
    _nan_scratch((c.nb, c.H, c.W, c.co))
    out.backward(dy.to(DEV))
    torch.cuda.synchronize()
    assert (K.DGRAD_POOL_CALLS - calls == 1) == (c.dgrad == "conv_dgrad_pool_k"), c.name
    got.update(dw=_f64(wd.grad.permute(0, 3, 1, 2)), db=_f64(bd.grad), dnw=_f64(nwd.grad))
    if c.dx:
        got["dx"] = _f64(xd.grad)
    if c.ipc:
        got.update(dgamma=_f64(film[0].grad), dbeta=_f64(film[1].grad))
    return got


@pytest.mark.parametrize("name", [c.name for c in cm.STAGE_CASES])
def test_stage_matches_float64(name, monkeypatch):
    c = cm.STAGE[name]
    _check_arms(c, monkeypatch)
    got = run_product_stage(c)
    ref = cm.run_stage_ref(c)
    print(name, {k: f"{e:.3g}/{b:.3g}" for k, (e, b) in cm.stage_errors(got, ref).items()})
    need = ("y", "amax", "dw", "db", "dnw") + (("dx",) if c.dx else ()) + (("dgamma", "dbeta") if c.ipc else ())
    cm.compare_stage(got, ref, name, need=need)


def run_product_up(c):
    from sdreamer import ops
    x, w, b, nw, dy = cm.up_inputs(c)
    xd, wd = x.to(DEV).requires_grad_(), _khwc(w).requires_grad_()
    bd, nwd = b.to(DEV).requires_grad_(), nw.to(DEV).requires_grad_()
    out = ops.UpConvFn.apply(xd, wd, bd)
    if not c.last:
        out = ops.rms_silu(out, nwd)
    _nan_scratch((c.nb, 2 * c.H, 2 * c.W, c.ci))  # the full-resolution input gradient sumpool2 reads
    out.backward(dy.to(DEV))
    torch.cuda.synchronize()
    got = dict(y=_f64(out), dx=_f64(xd.grad), dw=_f64(wd.grad.permute(0, 3, 1, 2)), db=_f64(bd.grad))
    if not c.last:
        got["dnw"] = _f64(nwd.grad)
    return got


@pytest.mark.parametrize("name", [c.name for c in cm.UP_CASES])
def test_upconv_matches_float64(name):
    from sdreamer import _native as nat
    c = cm.UP[name]
    assert cm.up_arms(c) == (c.fwd, c.wgrad, c.dgrad), f"{name} left its arm: {cm.up_arms(c)}"
    cm.check_plans(nat, c.nb, c.H, c.W, c.ci, c.co, c.k, 1)
    got = run_product_up(c)
    ref = cm.run_up_ref(c)
    print(name, {k: f"{e:.3g}/{b:.3g}" for k, (e, b) in cm.stage_errors(got, ref).items()})
    cm.compare_stage(got, ref, name, need=("y", "dx", "dw", "db") + (() if c.last else ("dnw",)))


@pytest.mark.parametrize("name", [c.name for c in cm.KERNEL_CASES])
def test_kernel_contraction_matches_float64(name):
    from sdreamer import _native as nat, kernels as K
    c = cm.KERNEL[name]
    assert cm.kernel_arms(c) == (c.arm, c.fast), f"{name} left its arm: {cm.kernel_arms(c)}"
    cm.check_plans(nat, c.nb, c.H, c.W, c.ci, c.co, c.k, c.ups)
    x, w, dout = (t.to(DEV) for t in cm.kernel_inputs(c))
    wk = _khwc(w)
    kr = cm.run_kernel_ref(c)

    def run(fast):
        if c.op == "fwd":
            return K.conv2d_fwd(x, wk, None, ups=c.ups)
        if c.op == "dgrad":
            return K.conv2d_dgrad(dout, wk, fast=fast)
        return K.conv2d_wgrad(x, dout, c.k, c.k, ups=c.ups, fast=fast)

    slow = run(False)
    rho = cm.compare_kernel(_f64(slow), kr, c.op, cm.F32_SLACK * kr["rho32"], f"{name} {c.arm}")
    bound = cm.F32_SLACK * kr["rho32"]
    print(f"{name}: {c.arm} ratio {rho:.3g} (float32 restatement {kr['rho32']:.3g}, bound {bound:.3g})")
    if c.fast:
        fast = run(True)
        assert not torch.equal(fast, slow), f"{name}: fast=True took the f32 arm"
        rho = cm.compare_kernel(_f64(fast), kr, c.op, cm.C_SPLIT, f"{name} {c.fast}")
        print(f"{name}: {c.fast} ratio {rho:.3g} (bound {cm.C_SPLIT})")
    elif c.op != "fwd":
        assert torch.equal(run(True), slow), f"{name}: fast=True left the f32 arm"


@pytest.mark.parametrize("H,W,C,nb,ipc", [(5, 4, 16, 2, 0), (4, 5, 24, 2, 0), (7, 7, 96, 3, 0), (21, 21, 32, 2, 2),
                                          (1, 6, 16, 2, 0), (6, 1, 16, 2, 2)])
def test_pool_rms_bwd_writes_the_dropped_edge(H, W, C, nb, ipc):
    """MaxPool2d(2) floors: an odd H or W leaves a last row / column in no window. Its conv gradient is zero, and
    pool_rms_bwd (plain and FiLM) writes it: the output buffer is not cleared beforehand. A one-row or one-column
    image has no window at all."""
    from sdreamer import kernels as K
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(nb, H, W, C, generator=g).to(DEV)
    nw = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    film = None
    if ipc:
        film = ((1 + 0.3 * torch.randn(nb // ipc, C, generator=g)).to(DEV),
                (0.3 * torch.randn(nb // ipc, C, generator=g)).to(DEV))
    y, pooled, amax, rstd = K.pool_rms_fwd(x, nw, film=film)
    dy = torch.randn(y.shape, generator=g).to(DEV)
    dnw = torch.zeros(C, device=DEV)
    _nan_scratch((nb, H, W, C))
    dx = K.pool_rms_bwd(pooled, amax, nw, rstd, dy, H, W, dnw, film=film)
    dx = dx[0] if ipc else dx
    torch.cuda.synchronize()
    assert not dx.isnan().any(), f"{int(dx.isnan().sum())} elements of the conv gradient were not written"
    Ho, Wo = H // 2, W // 2
    assert not dx[:, 2 * Ho:].any() and not dx[:, :, 2 * Wo:].any()
    assert (dx[:, :2 * Ho, :2 * Wo] != 0).sum().item() == nb * Ho * Wo * C  # one position per window and channel


def test_pool_rms_refuses_more_than_128_channels():
    """16 lanes x 8 channels per pooled pixel: C = 132 raises before anything is launched"""
    from sdreamer import _native as nat, kernels as K
    x = torch.zeros(1, 4, 4, 132, device=DEV)
    with pytest.raises(nat.NativeError):
        K.pool_rms_fwd(x, torch.ones(132, device=DEV))
    torch.cuda.synchronize()
    y, pooled, amax, rstd = K.pool_rms_fwd(x[..., :128].contiguous(), torch.ones(128, device=DEV))
    assert y.shape == (1, 2, 2, 128) and np.isfinite(_f64(y)).all()
