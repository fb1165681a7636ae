"""Wide conv encoder stages (a stage width of 129 .. 512 channels) against a float64 torch reference, on
tests/conv_models.py's reference, inputs, comparisons and bounds, unchanged (tests/wide_conv_models.py: the case
tables; tests/test_wide_conv_cpu.py checks the tie margins, the comparisons' discrimination and the host queries).

Per stage case, on the default switches and with the split-bf16 contractions switched off (kernels.FAST_GEMM False,
what SDREAMER_FAST_GEMM=0 sets): the forward, the saved argmax (equal at every window), and .backward(): dx, dW, db,
dnw and the FiLM gradients at compare_stage's caps (2e-5 forward, 5e-5 gradients, of max(max |ref|, 1)); NaN-filled
scratch shows every element written; a second call gives the same bits; a launch record (_native.PROBES) and the host
queries name the arm each contraction took.

Per kernel case: |err| <= c * contraction(|a|, |b|) + floor elementwise, c = 4e-5 on the split-bf16 arms and 8 x the
float32 restatement's own ratio on the f32 tiles; bwd-weight also with a forced slab count of 3 and adding into a
pre-filled gradient.
"""
import numpy as np
import pytest
import torch

import conv_models as cm
import wide_conv_models as wm

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _nan_scratch(*shapes):
    """allocate and free NaN-filled tensors of these shapes: the caching allocator hands the next torch.empty of a
    size one of them"""
    junk = [torch.full(s, float("nan"), device=DEV) for s in shapes for _ in range(3)]
    torch.cuda.synchronize()
    del junk


def _f64(t):
    return t.detach().double().cpu().numpy()


def _khwc(w):
    return w.permute(0, 2, 3, 1).contiguous().to(DEV)


Launches = wm.Launches


def _check_queries(c, cx):
    """the host queries name the wide arms for this shape, and every older fast arm refuses it"""
    from sdreamer import _native as nat, kernels as K
    q = nat.fns
    pad = c.k - 1 - (c.k - 1) // 2
    assert K.conv2d_dgrad_wide_takes(c.nb, c.H, c.W, c.co, cx, c.k, c.k, pad)
    want = wm.auto_slabs(c.nb, c.H, c.W, cx, c.co, c.k) if wm.wgrad_takes(cx, c.co) else 0
    assert K.conv2d_wgrad_wide_slabs(c.nb, c.H, c.W, cx, c.co, c.k, c.k) == want
    assert q["sd_conv2d_wgrad_bf16x3_slabs"](c.nb, c.H, c.W, cx, c.co, c.k, c.k, 0) <= 0
    assert q["sd_conv2d_wgrad_pool_slabs"](c.nb, c.H, c.W, cx, c.co, c.k, c.k) == 0
    cm.check_plans(nat, c.nb, c.H, c.W, cx, c.co, c.k)


def run_product_stage(c):
    from sdreamer import kernels as K, ops
    x, w, b, nw, gamma, beta, dy = cm.stage_inputs(c)
    wd, bd, nwd = _khwc(w).requires_grad_(), b.to(DEV).requires_grad_(), nw.to(DEV).requires_grad_()
    pad_shift = None
    if c.raw:  # the image's gradient is wanted: the stage pads (and un-pads) itself
        xd, pad_shift = x.to(DEV).requires_grad_(), 0.5
    else:
        xd = x.to(DEV).requires_grad_(c.dx)
    film = (gamma.to(DEV).requires_grad_(), beta.to(DEV).requires_grad_()) if c.ipc else None
    Ho, Wo = c.H // 2, c.W // 2
    with Launches() as rec:
        _nan_scratch((c.nb, c.H, c.W, c.co), (c.nb, Ho, Wo, c.co), (c.nb, Ho, Wo))
        if c.ipc:
            out = ops.FilmConvPoolNormFn.apply(xd, wd, bd, nwd, film[0], film[1], c.nchw, pad_shift)
        else:
            out = ops.ConvPoolNormFn.apply(xd, wd, bd, nwd, c.nchw, pad_shift)
        assert out.shape == dy.shape
        amax = out.grad_fn.saved_tensors[5]
        got = dict(y=_f64(out), amax=amax.cpu().numpy())
        _nan_scratch((c.nb, c.H, c.W, c.co), (c.nb, c.H, c.W, c.cx))
        out.backward(dy.to(DEV))
        torch.cuda.synchronize()
    got.update(dw=_f64(wd.grad.permute(0, 3, 1, 2)), db=_f64(bd.grad), dnw=_f64(nwd.grad))
    if c.dx:
        got["dx"] = _f64(xd.grad)
    if c.ipc:
        got.update(dgamma=_f64(film[0].grad), dbeta=_f64(film[1].grad))
    return got, rec


@pytest.mark.parametrize("fast", [True, False], ids=["x3", "f32"])
@pytest.mark.parametrize("name", [c.name for c in wm.STAGE_CASES])
def test_stage_matches_float64(name, fast, monkeypatch):
    from sdreamer import kernels as K, ops
    c = wm.STAGE[name]
    assert K.CONV6 and K.FAST_GEMM and ops.FUSED_POOL and ops.POOL_COMPACT, "the default switches"
    monkeypatch.setattr(K, "FAST_GEMM", fast)
    assert wm.stage_arms(c) == (c.fwd, c.wgrad, c.dgrad)
    _check_queries(c, c.cx)
    got, rec = run_product_stage(c)
    # the launch record: the forward on the f32 tiles + the wide row kernel, the backward on the arm `fast` names
    sfx = "_film" if c.ipc else ""
    assert rec.count("sd_pool_rms_wide_fwd" + sfx) == 1 and rec.count("sd_pool_rms_wide_bwd" + sfx) == 1
    assert not [n for n in rec.names if n.startswith("sd_pool_rms") and "_wide_" not in n]
    assert not [n for n in rec.names if n.startswith("sd_conv2d_fwd_pool")], "a fused forward was tried"
    x3w = fast and c.wgrad == wm.WGRAD  # (the first stage's bwd-weight stays on the f32 tiles)
    assert rec.count("sd_conv2d_wgrad_wide3") == int(x3w) and rec.count("sd_conv2d_wgrad") == int(not x3w)
    assert rec.count("sd_conv2d_dgrad_wide3") == int(fast and c.dx)
    assert rec.count("sd_conv2d_fwd") == 1 + int(c.dx and not fast)
    ref = cm.run_stage_ref(c)
    print(name, "x3" if fast else "f32", {k: f"{e:.3g}/{b:.3g}" for k, (e, b) in cm.stage_errors(got, ref).items()})
    need = ("y", "amax", "dw", "db", "dnw") + (("dx",) if c.dx else ()) + (("dgamma", "dbeta") if c.ipc else ())
    cm.compare_stage(got, ref, f"{name} fast={fast}", need=need)
    again, _ = run_product_stage(c)
    assert all(np.array_equal(got[k], again[k]) for k in got), "two calls differ"


@pytest.mark.parametrize("name", [c.name for c in wm.KERNEL_CASES])
def test_kernel_contraction_matches_float64(name):
    from sdreamer import kernels as K
    c = wm.KERNEL[name]
    assert K.FAST_GEMM and cm.kernel_arms(c) == (c.arm, "") and wm.wide_takes(c.ci, c.co)
    _check_queries(c, c.ci)
    x, w, dout = (t.to(DEV) for t in cm.kernel_inputs(c))
    wk = _khwc(w)
    kr = cm.run_kernel_ref(c)
    entry = "sd_conv2d_dgrad_wide3" if c.op == "dgrad" else "sd_conv2d_wgrad_wide3"

    def run(fast, **kw):
        _nan_scratch(tuple(kr["ref"].shape))
        with Launches() as rec:
            if c.op == "dgrad":
                out = K.conv2d_dgrad(dout, wk, fast=fast)
            else:
                out = K.conv2d_wgrad(x, dout, c.k, c.k, fast=fast, **kw)
        assert rec.count(entry) == int(fast and bool(c.fast)), f"{name}: fast={fast} ran {rec.names}"
        return out

    slow = run(False)
    bound = cm.F32_SLACK * kr["rho32"]
    rho = cm.compare_kernel(_f64(slow), kr, c.op, bound, f"{name} {c.arm}")
    print(f"{name}: {c.arm} ratio {rho:.3g} (float32 restatement {kr['rho32']:.3g}, bound {bound:.3g})")
    if not c.fast:  # not routed to the wide arm: fast=True stays on the f32 tiles
        assert torch.equal(run(True), slow), f"{name}: fast=True left the f32 arm"
        return
    fast = run(True)
    rho = cm.compare_kernel(_f64(fast), kr, c.op, cm.C_SPLIT, f"{name} {c.fast}")
    print(f"{name}: {c.fast} ratio {rho:.3g} (bound {cm.C_SPLIT})")
    assert torch.equal(run(True), fast), "two calls differ"
    if c.op == "wgrad":  # a forced slab count, and the launch adding into pre-filled parameter gradients
        pixels = c.nb * c.H * c.W
        forced = run(True, wide_slabs=wm.FORCED_SLABS)
        rho = cm.compare_kernel(_f64(forced), kr, c.op, cm.C_SPLIT, f"{name} {c.fast} in {wm.FORCED_SLABS} slabs")
        print(f"{name}: {wm.FORCED_SLABS} slabs ratio {rho:.3g}")
        if pixels > wm.slab_chunk(pixels, wm.FORCED_SLABS):
            assert not torch.equal(forced, fast), "the slab count changed nothing"
        g = torch.Generator().manual_seed(7)
        dw0, db0 = torch.randn(c.co, c.k, c.k, c.ci, generator=g), torch.randn(c.co, generator=g)
        dw, db = dw0.to(DEV), db0.to(DEV)
        assert run(True, wide_slabs=wm.FORCED_SLABS, acc=(dw, db, c.ci)) is None
        added = np.concatenate([(_f64(dw) - dw0.double().numpy()).reshape(c.co, -1),
                                (_f64(db) - db0.double().numpy())[:, None]], 1)
        rho = cm.compare_kernel(added, kr, c.op, cm.C_SPLIT, f"{name} {c.fast} acc")
        print(f"{name}: acc ratio {rho:.3g}")


def test_fast_gemm_off_keeps_wide_shapes_on_the_f32_tiles(monkeypatch):
    from sdreamer import kernels as K
    c = wm.KERNEL["kd_154_231"]
    x, w, dout = (t.to(DEV) for t in cm.kernel_inputs(c))
    slow = K.conv2d_dgrad(dout, _khwc(w), fast=False)
    monkeypatch.setattr(K, "FAST_GEMM", False)
    with Launches() as rec:
        assert torch.equal(K.conv2d_dgrad(dout, _khwc(w)), slow)
        assert torch.equal(K.conv2d_wgrad(x, dout, c.k, c.k), K.conv2d_wgrad(x, dout, c.k, c.k, fast=False))
    assert not [n for n in rec.names if "wide3" in n and not n.endswith(("_ok", "_slabs"))]


@pytest.mark.parametrize("H,W,C,nb,ipc", [(5, 4, 129, 2, 0), (4, 5, 231, 2, 0), (7, 7, 512, 3, 0), (9, 7, 154, 2, 2),
                                          (1, 6, 130, 2, 0), (6, 1, 300, 2, 2)])
def test_wide_pool_rms_bwd_writes_the_dropped_edge(H, W, C, nb, ipc):
    """MaxPool2d(2) floors: an odd H or W leaves a last row / column in no window. Its conv gradient is zero, and
    the wide backward (plain and FiLM) writes it, as the narrow one does."""
    from sdreamer import kernels as K
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(nb, H, W, C, generator=g).to(DEV)
    nw = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    film = None
    if ipc:
        film = ((1 + 0.3 * torch.randn(nb // ipc, C, generator=g)).to(DEV),
                (0.3 * torch.randn(nb // ipc, C, generator=g)).to(DEV))
    y, pooled, amax, rstd = K.pool_rms_wide_fwd(x, nw, film=film)
    dy = torch.randn(y.shape, generator=g).to(DEV)
    dnw = torch.zeros(C, device=DEV)
    _nan_scratch((nb, H, W, C))
    dx = K.pool_rms_wide_bwd(pooled, amax, nw, rstd, dy, H, W, dnw, film=film)
    dx = dx[0] if ipc else dx
    torch.cuda.synchronize()
    assert not dx.isnan().any(), f"{int(dx.isnan().sum())} elements of the conv gradient were not written"
    Ho, Wo = H // 2, W // 2
    assert not dx[:, 2 * Ho:].any() and not dx[:, :, 2 * Wo:].any()
    assert (dx[:, :2 * Ho, :2 * Wo] != 0).sum().item() == nb * Ho * Wo * C


def test_wide_pool_rms_propagates_nan_like_the_narrow_kernel():
    """the argmax is NaN-propagating: a NaN in a window is the window's maximum, at its position"""
    from sdreamer import kernels as K
    x = torch.randn(1, 2, 2, 200, generator=torch.Generator().manual_seed(3)).to(DEV)
    x[0, 1, 0, 150] = float("nan")
    y, pooled, amax, rstd = K.pool_rms_wide_fwd(x, torch.ones(200, device=DEV))
    assert pooled[0, 0, 0, 150].isnan() and int(amax[0, 0, 0, 150]) == 2 and not pooled[0, 0, 0, :150].isnan().any()


def test_wide_entries_refuse_513_channels():
    from sdreamer import _native as nat, kernels as K
    x = torch.zeros(1, 4, 4, 513, device=DEV)
    with pytest.raises(nat.NativeError):
        K.pool_rms_wide_fwd(x, torch.ones(513, device=DEV))
    with pytest.raises(nat.NativeError):
        K.pool_rms_wide_fwd(x[..., :128].contiguous(), torch.ones(128, device=DEV))
    torch.cuda.synchronize()


def test_wide_row_kernels_past_2_gib():
    """The real first-stage size x (1024, 64, 64, 154): 646 M floats, element offsets above 2^31 bytes. Forward and
    backward, the last two images bit for bit against a run on those two images alone."""
    from sdreamer import kernels as K
    Nb, H, W, C = 1024, 64, 64, 154
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(Nb, H, W, C, device=DEV, generator=g)
    assert x.numel() * 4 > 2 ** 31
    nw = 1 + 0.1 * torch.randn(C, device=DEV, generator=g)
    dy = torch.randn(Nb, H // 2, W // 2, C, device=DEV, generator=g)
    y, pooled, amax, rstd = K.pool_rms_wide_fwd(x, nw)
    dx = K.pool_rms_wide_bwd(pooled, amax, nw, rstd, dy, H, W, torch.zeros(C, device=DEV))
    ty, tp, ta, tr = K.pool_rms_wide_fwd(x[-2:].contiguous(), nw)
    tdx = K.pool_rms_wide_bwd(tp, ta, nw, tr, dy[-2:].contiguous(), H, W, torch.zeros(C, device=DEV))
    torch.cuda.synchronize()
    for name, big, small in (("y", y, ty), ("pooled", pooled, tp), ("amax", amax, ta), ("rstd", rstd, tr),
                             ("dx", dx, tdx)):
        assert torch.equal(big[-2:], small), name
    assert y[-2:].isfinite().all() and dx[-2:].isfinite().all() and (dx[-2:] != 0).sum().item() == 2 * 32 * 32 * C
