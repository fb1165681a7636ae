"""Autograd wrappers: each differentiable piece of the update owns a HIP forward AND a HIP backward.

Parameter gradients are accumulated straight into `param.grad` (normally a view into the flat gradient arena,
see sdreamer/optim.py) by the backward kernels (GEMM beta=1 / accumulate flags) instead of being returned to
autograd, so weight gradients never take an extra allocation + add pass. Input gradients are returned normally.
"""
from __future__ import annotations

import os

import torch

from . import kernels as k


# ConvEncoder stages run conv + pool + norm as one launch where the shape allows (SDREAMER_FUSED_POOL=0: two launches)
FUSED_POOL = os.environ.get("SDREAMER_FUSED_POOL", "1") != "0"


_GRAD_SINK = None  # a dict while a backward's parameter gradients are routed to scratch buffers (grad_sink_scope)


def grad_buf(param):
    if _GRAD_SINK is not None:  # id(param) -> scratch, dropped when the backward ends: param.grad is never touched
        buf = _GRAD_SINK.get(id(param))
        if buf is None:
            buf = _GRAD_SINK[id(param)] = torch.zeros_like(param)
        return buf
    if param.grad is None:
        param.grad = torch.zeros_like(param)
    return param.grad


def close_grad_sink():
    global _GRAD_SINK
    _GRAD_SINK = None


class grad_sink_scope:
    """Within this context every backward's parameter gradients go to scratch buffers (see grad_buf)."""

    def __enter__(self):
        global _GRAD_SINK
        self.prev, _GRAD_SINK = _GRAD_SINK, ({} if _GRAD_SINK is None else _GRAD_SINK)

    def __exit__(self, *exc):
        global _GRAD_SINK
        _GRAD_SINK = self.prev


class GradSinkFn(torch.autograd.Function):
    """Identity on the outputs of a forward whose backward must leave every parameter gradient alone (the posterior
    handed out by Dreamer.posterior(with_grad=True): only the gradient with respect to the observation is wanted).
    Its backward runs before any node of that forward: it routes grad_buf to scratch buffers and asks the autograd
    engine to end the routing when the whole backward has finished."""

    @staticmethod
    def forward(ctx, *xs):
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for x in xs)

    @staticmethod
    def backward(ctx, *gs):
        global _GRAD_SINK
        if _GRAD_SINK is None:
            _GRAD_SINK = {}
            torch.autograd.Variable._execution_engine.queue_callback(close_grad_sink)
        return gs


def _flat(x):
    return x.reshape(-1, x.shape[-1])


# ------------------------------------------------------------------------------------------------- dense layers
_DEFER = None  # a list while defer_wgrads is active


class defer_wgrads:
    """Within this context LinearFn's backward computes the input gradient immediately and queues its weight / bias
    gradient contractions in `bucket`; flush_wgrads runs them later, possibly on another stream (the replay-value
    loss's value-head weight gradients run on the side stream, off the path to the posterior backward)."""

    def __init__(self, bucket):
        self.bucket = bucket

    def __enter__(self):
        global _DEFER
        self.prev, _DEFER = _DEFER, self.bucket
        return self.bucket

    def __exit__(self, *exc):
        global _DEFER
        _DEFER = self.prev


def flush_wgrads(bucket):
    """Run the queued weight-gradient work on the current stream (inputs marked as used by it)."""
    st = torch.cuda.current_stream()
    eager = not torch.cuda.is_current_stream_capturing()  # captured phases keep their tensors in the graph pools
    for fn, tensors in bucket:
        if eager:
            for t in tensors:
                t.record_stream(st)
        fn()
    bucket.clear()


class DxSink:
    """One input-gradient buffer shared by several linear layers that read the same tensor x (the world-model heads
    and the replay value head on the posterior feat, dreamer.py:571-660): each layer's backward adds its x gradient
    into `buf` inside its own GEMM (beta = 1 after the first writer) and returns no gradient to autograd, so the
    pairwise autograd adds, the slice-backward copies of the concatenated feat and the leaf-gradient copies are never
    launched. Mark an input with `sink(x, s)`; `written` tells whether any layer's gradient arrived."""

    def __init__(self, like):
        self.buf = torch.empty(like.shape, dtype=torch.float32, device=like.device)
        self.written = False


def sink(x, s):
    """x with its linear layers' input gradients routed into DxSink s (the attribute does not survive a view)"""
    x._dx_sink = s
    return x


class LinearFn(torch.autograd.Function):
    """nn.Linear (y = x W^T + b). Gradients on the split-bf16 GEMM (k.gemm fast=True, ~1e-5 relative); the forward
    too when `fast` (imagined-trajectory heads: no sampled index depends on them). An input marked with a DxSink gets
    its gradient accumulated there instead of returned."""

    @staticmethod
    def forward(ctx, x, w, b, fast=False):
        x2 = _flat(x).contiguous()
        y = k.mm(x2, w.t(), bias=b, fast=fast)
        ctx.save_for_backward(x2, w, b)
        ctx.in_shape = x.shape
        ctx.dx_sink = getattr(x, "_dx_sink", None)
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w, b = ctx.saved_tensors
        dy2 = _flat(dy).contiguous()
        dx = None
        sk = ctx.dx_sink
        if sk is not None:
            k.mm(dy2, w, out=sk.buf.view(-1, w.shape[1]), beta=1.0 if sk.written else 0.0, fast=True)
            sk.written = True
        elif ctx.needs_input_grad[0]:
            dx = k.mm(dy2, w, fast=True).view(ctx.in_shape)

        def wgrad():
            if w.requires_grad:  # dW (+ db in the same launch)
                k.wgrad(dy2, x2, grad_buf(w), grad_buf(b) if (b is not None and b.requires_grad) else None)
            elif b is not None and b.requires_grad:
                k.colsum(dy2, grad_buf(b), accumulate=True)

        if _DEFER is not None:
            _DEFER.append((wgrad, (dy2, x2)))
        else:
            wgrad()
        return dx, None, None, None


class LinearPreFn(torch.autograd.Function):
    """A linear layer whose forward output h = x W^T + b was already computed elsewhere (the imagination's fp32 actor
    layer 0, the imagined heads' batched first layers): forward returns h0 as the layer's output, backward accumulates
    the weight / bias gradients exactly as LinearFn does (split-bf16 dW = dh^T x, column sums for db). x is a detached
    input (imagined features): no input gradient."""

    @staticmethod
    def forward(ctx, h0, x, w, b):
        ctx.save_for_backward(_flat(x).contiguous(), w, b)
        return h0.view_as(h0)

    @staticmethod
    def backward(ctx, dy):
        x2, w, b = ctx.saved_tensors
        dy2 = _flat(dy).contiguous()

        def wgrad():
            if w.requires_grad:  # dW (+ db in the same launch)
                k.wgrad(dy2, x2, grad_buf(w), grad_buf(b) if (b is not None and b.requires_grad) else None)
            elif b is not None and b.requires_grad:
                k.colsum(dy2, grad_buf(b), accumulate=True)

        if _DEFER is not None:
            _DEFER.append((wgrad, (dy2, x2)))
        else:
            wgrad()
        return None, None, None, None


class PairFirstFn(torch.autograd.Function):
    """The first layer (Linear -> RMSNorm -> SiLU) of two MLPs on the same detached input x whose linear outputs
    h0a, h0b were computed elsewhere: the imagined actor's (the imagination's fp32 layer 0) and the value head's (the
    imagined heads' batched first layer), dreamer.py:607,613. Forward = the two norms (as RmsSiluFn). Backward: both
    norms' input gradients into the two column blocks of one (R, Ua + Ub) buffer, then ONE split-bf16 weight-gradient
    GEMM over it (sd_gemm_bf16x3_wgrad2) — x (H*N x feat, 157 MB at the bench config) is read once instead of once per
    head, and its K chunks are twice as long. The two weight gradients must lie back to back (Dreamer._arena_order);
    otherwise two GEMMs over the buffer's column blocks."""

    @staticmethod
    def forward(ctx, h0a, h0b, x, wa, ba, na, wb, bb, nb):
        h0a, h0b = h0a.contiguous(), h0b.contiguous()
        ya, ra = k.rmsnorm_fwd(h0a, na, act=1)
        yb, rb = k.rmsnorm_fwd(h0b, nb, act=1)
        ctx.save_for_backward(h0a, h0b, ra, rb, _flat(x).contiguous(), wa, ba, na, wb, bb, nb)
        return ya, yb

    @staticmethod
    def backward(ctx, dya, dyb):
        h0a, h0b, ra, rb, x2, wa, ba, na, wb, bb, nb = ctx.saved_tensors
        R, Ua = h0a.shape
        Ub = h0b.shape[1]
        buf = torch.empty(R, Ua + Ub, dtype=torch.float32, device=h0a.device)
        for h0, nw, r, dy, cols in ((h0a, na, ra, dya, slice(0, Ua)), (h0b, nb, rb, dyb, slice(Ua, Ua + Ub))):
            if dy is None:
                buf[:, cols].zero_()
            else:
                k.rmsnorm_bwd(h0, nw, r, dy, act=1, dx=buf[:, cols], dw=grad_buf(nw) if nw.requires_grad else None)

        def wgrad():
            ga, gb = grad_buf(wa), grad_buf(wb)
            if not (gb.data_ptr() == ga.data_ptr() + ga.numel() * ga.element_size() and ga.is_contiguous() and
                    gb.is_contiguous() and k.wgrad2(buf, x2, ga.as_strided((Ua + Ub, ga.shape[1]), (ga.shape[1], 1)),
                                                    grad_buf(ba), grad_buf(bb), Ua) is not False):
                k.wgrad(buf[:, :Ua], x2, ga, grad_buf(ba))
                k.wgrad(buf[:, Ua:], x2, gb, grad_buf(bb))

        if _DEFER is not None:
            _DEFER.append((wgrad, (buf, x2)))
        else:
            wgrad()
        return (None,) * 9


class RmsSiluFn(torch.autograd.Function):
    """nn.RMSNorm(eps=1e-4, or `eps`) followed by SiLU (act=1) or nothing (act=0). The backward reads the saved rstd,
    so eps enters the forward only."""

    @staticmethod
    def forward(ctx, x, w, act, eps=None):
        x = x.contiguous()
        y, rstd = k.rmsnorm_fwd(x, w, act=act, eps=eps)
        ctx.save_for_backward(x, w, rstd)
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, rstd = ctx.saved_tensors
        dw = grad_buf(w) if w.requires_grad else None
        dx = k.rmsnorm_bwd(x, w, rstd, dy.contiguous(), act=ctx.act, dw=dw)
        return dx, None, None, None


class BlockLinearFn(torch.autograd.Function):
    """BlockLinear (networks.py:24-56) with the weight kept packed as (G, O/G, I/G)."""

    @staticmethod
    def forward(ctx, x, wp, b):
        G, Og, Ig = wp.shape
        x2 = _flat(x).contiguous()
        M = x2.shape[0]
        y = torch.empty(M, G * Og, dtype=torch.float32, device=x.device)
        k.gemm(x2.view(M, G, Ig).permute(1, 0, 2), wp.transpose(1, 2), y.view(M, G, Og).permute(1, 0, 2),
               bias=b.view(G, Og))
        ctx.save_for_backward(x2, wp, b)
        ctx.in_shape = x.shape
        return y.view(*x.shape[:-1], G * Og)

    @staticmethod
    def backward(ctx, dy):
        x2, wp, b = ctx.saved_tensors
        G, Og, Ig = wp.shape
        M = x2.shape[0]
        dy2 = _flat(dy).contiguous()
        dyv = dy2.view(M, G, Og).permute(1, 0, 2)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, G * Ig, dtype=torch.float32, device=dy.device)
            k.gemm(dyv, wp, dx.view(M, G, Ig).permute(1, 0, 2), fast=True)
            dx = dx.view(ctx.in_shape)
        if wp.requires_grad:
            k.gemm(dyv.transpose(1, 2), x2.view(M, G, Ig).permute(1, 0, 2), grad_buf(wp), beta=1.0, fast=True)
        if b.requires_grad:
            k.colsum(dy2, grad_buf(b), accumulate=True)
        return dx, None, None


def linear(x, w, b=None, fast=False):
    return LinearFn.apply(x, w, b, fast)


def linear_pre(h0, x, w, b=None):
    return LinearPreFn.apply(h0, x, w, b)


def rms_silu(x, w, act=1, eps=None):
    return RmsSiluFn.apply(x, w, act, eps)


def block_linear(x, wp, b):
    return BlockLinearFn.apply(x, wp, b)


# ------------------------------------------------------------------------------------------------- conv
# SDREAMER_POOL_COMPACT=0: every stage's backward through the full-resolution conv gradient (benchmark / test knob)
POOL_COMPACT = os.environ.get("SDREAMER_POOL_COMPACT", "1") != "0"


class CatIntoFn(torch.autograd.Function):
    """torch.cat([a, b], -1) written into a caller-owned buffer (holder[0]) and returned with autograd: RSSM.get_feat
    (rssm.py:211-217) straight into the imagination's start slot, so the start state is never copied again."""

    @staticmethod
    def forward(ctx, a, b, holder):
        out = holder[0]
        na, nb, F = a.shape[-1], b.shape[-1], out.shape[-1]
        rows = a.numel() // na
        if out.stride(-1) != 1 or out.numel() != rows * F or na + nb != F or not (a.is_contiguous() and b.is_contiguous()):
            torch.cat([a, b], -1, out=out)
        else:  # both halves in one sd_layout_copies_run launch (row stride F into the slot)
            base = out.reshape(rows, F)
            k.layout_copies([(a, base, 1, rows, na, 0, na, na, 1, F), (b, base[:, na:], 1, rows, nb, 0, nb, nb, 1, F)])
        ctx.split = na
        ctx.set_materialize_grads(False)  # consumers that route their gradient into a DxSink send none here
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None
        return g[..., :ctx.split], g[..., ctx.split:], None


def _pad_last(w, n):
    """w (..., c) -> (..., n) zero-padded, one sd_layout_copies_run launch"""
    wc = w.contiguous()
    out = torch.empty(*w.shape[:-1], n, dtype=w.dtype, device=w.device)
    rows = wc.numel() // w.shape[-1]
    k.layout_copies([(wc, out, 1, rows, w.shape[-1], 0, w.shape[-1], n, 1)])
    return out


def _stage_input(x, w, pad_shift):
    """-> (the conv's input, the weight it runs with). pad_shift given: x is the raw image (its real channel count);
    the input x - pad_shift zero-padded to a multiple of four channels is formed here, so the stage's backward hands
    autograd a gradient of the image's own shape and no padded gradient exists."""
    if pad_shift is not None:
        x = k.pad_channels(x.contiguous(), (x.shape[-1] + 3) // 4 * 4, float(pad_shift))
    return x, (w if x.shape[-1] == w.shape[-1] else _pad_last(w, x.shape[-1]))


def _stage_wide(w):
    """The one place a stage is sent to the wide row kernels (k.pool_rms_wide_fwd / k.pool_rms_wide_bwd): more output
    channels than the narrow ones hold. No fused forward and no pooled-gradient route exists at these widths."""
    return w.shape[0] > k.WIDE_ROWS_MIN


def _stage_route(need_dx, x, w):
    """The one place a stage's backward route is chosen, for the conv input x (after _stage_input) and the weight w as
    the module holds it: "first", "x3", "full" or "wide".
    wide: _stage_wide(w). The full route on the wide row kernel; k.conv2d_wgrad / k.conv2d_dgrad pick their wide arms.
    first: the first stage. Its f32 / split-bf16 pooled bwd-weight (k.conv2d_wgrad_pool) takes the shape, and the input
    gradient is not wanted or x is channel-padded and k.conv2d_dgrad_pool takes it: both expand the pooled gradient +
    argmax themselves.
    x3: stages 2-3. The split-bf16 bwd-weight has its pooled form at its plan (k.conv2d_wgrad_pooled), and the input
    gradient is not wanted or has one too (k.conv2d_dgrad_pooled); every gradient is the full route's bit for bit.
    full: through the full-resolution conv gradient (3/4 zeros), which the other two never write or read."""
    Nb, H, W, Cx = x.shape
    Co, kh, kw, Ci = w.shape
    if _stage_wide(w):
        return "wide"
    if not POOL_COMPACT:
        return "full"
    if k.conv2d_wgrad_pool_slabs(x, Co, kh, kw) > 0 and (
            not need_dx or (Cx != Ci and k.conv2d_dgrad_pool_takes(H, W, Co, Ci, kh, kw))):
        return "first"
    if k.conv2d_wgrad_pooled_slabs(x, Co, kh, kw) > 0 and (
            not need_dx or (Cx == Ci and k.conv2d_dgrad_pooled_takes(H, W, Co, Ci, kh, kw))):
        return "x3"
    return "full"


def _stage_dx(ctx, x, w, dconv, dpool, amax, x3=False):
    """The stage's input gradient in the shape autograd expects: the raw image's channels (pad_shift route) or x's.
    dconv None: from the pooled gradient (x3: on the direct split-bf16 kernel); else conv2d_dgrad, on the zero-padded
    weight when x carries pad channels (their gradient is zero: they meet zero weights only)."""
    Cx, Ci = x.shape[-1], w.shape[-1]
    if dconv is None:
        dx = k.conv2d_dgrad_pooled(dpool, amax, w) if x3 else k.conv2d_dgrad_pool(dpool, amax, w)
        if dx is None:
            raise k.nat.NativeError("the pooled input gradient refused a shape its query accepted")
    else:
        dx = k.conv2d_dgrad(dconv, w if Cx == Ci else _pad_last(w, Cx))
    want = ctx.raw_c if ctx.raw_c is not None else Cx
    if dx.shape[-1] > want:
        dx = dx[..., :want].contiguous()
    elif dx.shape[-1] < want:
        dx = _pad_last(dx, want)
    return dx


def _stage_wgrad(x, dconv, dpool, amax, kh, kw, acc):
    """The stage's split-bf16 bwd-weight, from the full-resolution conv gradient or (dpool set) from the pooled one;
    queued while ops.defer_wgrads is active (only the data gradient continues the backward chain). Neither given: the
    first stage's pooled route has run its own already."""
    if dconv is None and dpool is None:
        return
    if dpool is not None:
        wgrad, keep = (lambda: k.conv2d_wgrad_pooled(x, dpool, amax, kh, kw, acc=acc)), (x, dpool, amax)
    else:
        wgrad, keep = (lambda: k.conv2d_wgrad(x, dconv, kh, kw, acc=acc)), (x, dconv)
    if _DEFER is not None:
        _DEFER.append((wgrad, keep))
    else:
        wgrad()


class ConvPoolNormFn(torch.autograd.Function):
    """One ConvEncoder stage: Conv2dSamePad -> MaxPool2d(2) -> RMSNorm2D -> [gamma * x + beta] -> SiLU
    (networks.py:201-216; the FiLM stage when gamma / beta are given), NHWC. Forward on the exact f32 MFMA kernels (the
    posterior samples depend on it); both backward contractions on the split-bf16 kernels (k.conv2d_wgrad /
    k.conv2d_dgrad, ~1e-5 relative), on the route _stage_route names.
    gamma / beta are (rows, Co), one row per Nb / rows consecutive images (a batch row's T frames), applied in the same
    kernels' epilogue; their gradients are returned to autograd (the FiLM generator continues the chain), every
    parameter gradient is accumulated. With gamma = 1 and beta = 0 every output and gradient equals the plain stage's
    bit for bit."""

    @staticmethod
    def forward(ctx, x, w, b, nw, nchw_flat, pad_shift=None, gamma=None, beta=None):
        # x may carry zero-padded channels (first layer: 3 -> 4); the weight is padded to match
        ctx.raw_c = x.shape[-1] if pad_shift is not None else None
        x, wk = _stage_input(x, w, pad_shift)
        film = None if gamma is None else (gamma.contiguous(), beta.contiguous())
        wide = _stage_wide(w)
        fused = None
        if FUSED_POOL and not wide:
            fused = k.conv2d_fwd_pool(x.contiguous(), wk, b, nw, nchw_flat=nchw_flat, film=film)
        if fused is None:
            conv = k.conv2d_fwd(x.contiguous(), wk, b)
            fused = (k.pool_rms_wide_fwd if wide else k.pool_rms_fwd)(conv, nw, nchw_flat=nchw_flat, film=film)
            del conv
        y, pooled, amax, rstd = fused
        ctx.save_for_backward(x, w, b, nw, pooled, amax, rstd, *(film or ()))
        ctx.nchw_flat = nchw_flat
        if nchw_flat:
            return y.view(y.shape[0], -1)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, b, nw, pooled, amax, rstd, *film = ctx.saved_tensors
        film = tuple(film) or None
        Nb, H, W, _ = x.shape
        Co, kh, kw, Ci = w.shape
        need_dx = ctx.needs_input_grad[0]
        acc = (grad_buf(w), grad_buf(b), Ci)  # the bwd-weight launches add into the gradients themselves
        route = _stage_route(need_dx, x, w)
        if route == "wide":
            d = k.pool_rms_wide_bwd(pooled, amax, nw, rstd, dy.contiguous(), H, W, grad_buf(nw),
                                    nchw_flat=ctx.nchw_flat, film=film)
            route = "full"  # from here on the full-resolution conv gradient's route
        elif route == "full":
            d = k.pool_rms_bwd(pooled, amax, nw, rstd, dy.contiguous(), H, W, grad_buf(nw), nchw_flat=ctx.nchw_flat,
                               film=film)
        else:
            d = k.pool_rms_bwd_compact(pooled, amax, nw, rstd, dy.contiguous(), grad_buf(nw), nchw_flat=ctx.nchw_flat,
                                       film=film)
        d, dgamma, dbeta = d if film else (d, None, None)
        dconv, dpool = (d, None) if route == "full" else (None, d)
        if route == "first":
            k.conv2d_wgrad_pool(x, dpool, amax, kh, kw, acc=acc)
        _stage_wgrad(x, dconv, dpool if route == "x3" else None, amax, kh, kw, acc)
        dx = _stage_dx(ctx, x, w, dconv, dpool, amax, route == "x3") if need_dx else None
        return dx, None, None, None, None, None, dgamma, dbeta


class FilmConvPoolNormFn:
    """The FiLM stage under its earlier name and argument order (gamma, beta before nchw_flat): no function of its
    own, ConvPoolNormFn with gamma / beta."""

    @staticmethod
    def apply(x, w, b, nw, gamma, beta, nchw_flat, pad_shift=None):
        return ConvPoolNormFn.apply(x, w, b, nw, nchw_flat, pad_shift, gamma, beta)


class RowBiasSiluFn(torch.autograd.Function):
    """silu(x[n] + u[n // T]): x (N, E), u (N // T, E) or None (plain nn.SiLU). The text gate's first layer is
    cat[v, tp] . W^T = v . Wv^T + (tp . Wt^T + b)[n // T]: the tp half is a B-row GEMM added here per batch row, so
    neither the concatenation nor an expanded tp exists. du sums each batch row's T rows in row order."""

    @staticmethod
    def forward(ctx, x, u, T):
        x = x.contiguous()
        y = k.rowbias_silu_fwd(x, u, T)
        ctx.save_for_backward(x, u)
        ctx.T = T
        return y

    @staticmethod
    def backward(ctx, dy):
        x, u = ctx.saved_tensors
        dx, du = k.rowbias_silu_bwd(x, u, dy.contiguous(), ctx.T, need_du=u is not None and ctx.needs_input_grad[1])
        return dx, du, None


class TextGateFn(torch.autograd.Function):
    """out = (1 - g) v + g tp[n // T], g = sigmoid(a): v, a (N, E), tp (N // T, E) read by row n // T. Returns
    (out, g); g carries no gradient (a diagnostic: its mean / unbiased std are Stat metrics)."""

    @staticmethod
    def forward(ctx, v, a, tp, T):
        v, tp = v.contiguous(), tp.contiguous()
        out, g = k.text_gate_fwd(v, a, tp, T)
        ctx.save_for_backward(v, g, tp)
        ctx.T = T
        ctx.mark_non_differentiable(g)
        return out, g

    @staticmethod
    def backward(ctx, d, _dg):
        v, g, tp = ctx.saved_tensors
        dv, da, dtp = k.text_gate_bwd(v, g, tp, d.contiguous(), ctx.T)
        return dv, da, dtp, None


class GateFirstFn(torch.autograd.Function):
    """The text gate's first layer h = silu(cat[v, tp[n // T]] . W^T + b) without the concatenation: W (E, 2E) is read
    as its v half and its tp half in place, pre = v . Wv^T over the N rows and u = tp . Wt^T + b over the B context
    rows, h = silu(pre + u[n // T]). Forward on the exact f32 path (the posterior's input depends on it); the input
    gradients and both halves of dW (accumulated into W's gradient in place) on the split-bf16 path."""

    @staticmethod
    def forward(ctx, v, tp, w, b, T):
        E = w.shape[0]
        v2, tp2 = v.contiguous(), tp.contiguous()
        pre = k.mm(v2, w[:, :E].t())
        u = k.mm(tp2, w[:, E:].t(), bias=b)
        ctx.save_for_backward(v2, tp2, w, b, pre, u)
        ctx.T = T
        return k.rowbias_silu_fwd(pre, u, T)

    @staticmethod
    def backward(ctx, dh):
        v2, tp2, w, b, pre, u = ctx.saved_tensors
        E = w.shape[0]
        dpre, du = k.rowbias_silu_bwd(pre, u, dh.contiguous(), ctx.T)
        dv = k.mm(dpre, w[:, :E], fast=True) if ctx.needs_input_grad[0] else None
        dtp = k.mm(du, w[:, E:], fast=True) if ctx.needs_input_grad[1] else None
        if w.requires_grad:
            gw = grad_buf(w)
            k.wgrad(dpre, v2, gw[:, :E])
            k.wgrad(du, tp2, gw[:, E:], grad_buf(b) if b.requires_grad else None)
        elif b.requires_grad:
            k.colsum(du, grad_buf(b), accumulate=True)
        return dv, dtp, None, None, None


def rowbias_silu(x, u=None, T=1):
    return RowBiasSiluFn.apply(x, u, T)


def text_gate(v, a, tp, T):
    return TextGateFn.apply(v, a, tp, T)


class UpConvFn(torch.autograd.Function):
    """nn.Upsample(2, nearest) -> Conv2dSamePad (ConvDecoder, networks.py:259-265), NHWC, no materialised upsample."""

    @staticmethod
    def forward(ctx, x, w, b):
        y = k.conv2d_fwd(x.contiguous(), w, b, ups=1)
        ctx.save_for_backward(x, w, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, b = ctx.saved_tensors
        Co, kh, kw, Ci = w.shape
        dy = dy.contiguous()
        k.conv2d_wgrad(x, dy, kh, kw, ups=1, acc=(grad_buf(w), grad_buf(b), Ci))
        dx = None
        if ctx.needs_input_grad[0]:
            du = k.conv2d_dgrad(dy, w)
            dx = k.sumpool2(du)
        return dx, None, None


# ------------------------------------------------------------------------------------------------- distributions
class KLFn(torch.autograd.Function):
    """RSSM.kl_loss (rssm.py:222-230): returns (dyn_row, rep_row) = clip(sum_S KL, min=free) for every row."""

    @staticmethod
    def forward(ctx, post, prior, free, S, K):
        post, prior = post.contiguous(), prior.contiguous()
        kl, dyn, rep = k.kl_rows(post, prior, S, K, free=free)  # the clamped copies come from the same launch
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(post, prior, kl)
        ctx.free, ctx.S, ctx.K = free, S, K
        return dyn, rep

    @staticmethod
    def backward(ctx, g_dyn, g_rep):
        post, prior, kl = ctx.saved_tensors
        rows = kl.numel()
        d_post = torch.empty_like(post) if ctx.needs_input_grad[0] else None
        d_prior = torch.empty_like(prior) if ctx.needs_input_grad[1] else None
        gd = g_dyn.contiguous() if g_dyn is not None else None
        gr = g_rep.contiguous() if g_rep is not None else None
        k.nat.call("sd_kl_bwd", k.p(post), k.p(prior), k.p(kl), k.p(gr), k.p(gd), float(ctx.free), k.p(d_post),
                   k.p(d_prior), rows, ctx.S, ctx.K, 0, 0, k.stream())
        return d_post, d_prior, None, None, None


class LossTermsFn(torch.autograd.Function):
    """The world-model loss dict and its weighted total (dreamer.py:571-576): term i = coefs[i] * mean(xs[i]), total =
    sum_i scales[i] * term_i in order. One launch forward (sd_loss_terms_fwd), one backward (every input's gradient,
    sd_loss_terms_bwd), instead of a reduce + scalar-op chain per term. Returns (total (), terms (n,))."""

    @staticmethod
    def forward(ctx, coefs, scales, *xs):
        xs = [x.contiguous() for x in xs]
        dev = xs[0].device
        terms = torch.empty(len(xs), dtype=torch.float32, device=dev)
        total = torch.empty(1, dtype=torch.float32, device=dev)
        k.loss_terms(xs, coefs, scales, terms, total)
        ctx.coefs, ctx.scales = list(coefs), list(scales)
        ctx.shapes = [x.shape for x in xs]
        ctx.dev = dev
        ctx.set_materialize_grads(False)  # an unused output's gradient stays None (no zeros launch)
        return total[0], terms

    @staticmethod
    def backward(ctx, g_total, g_terms):
        n = len(ctx.shapes)
        grads = [torch.empty(sh, dtype=torch.float32, device=ctx.dev) if ctx.needs_input_grad[2 + i] else None
                 for i, sh in enumerate(ctx.shapes)]
        if any(g is not None for g in grads):
            gt = g_total.reshape(1).contiguous() if g_total is not None else None
            gm = g_terms.contiguous() if g_terms is not None else None
            k.loss_terms_bwd([torch.Size(sh).numel() for sh in ctx.shapes], ctx.coefs, ctx.scales, grads, gt, gm)
        return (None, None) + tuple(grads[:n])


class TwoHotLogProbFn(torch.autograd.Function):
    """TwoHot.log_prob (distributions.py:100-129) for symexp bins; target detached."""

    @staticmethod
    def forward(ctx, logits, bins, target):
        NB = logits.shape[-1]
        l2 = _flat(logits).contiguous()
        t = target.reshape(-1).contiguous()
        out = torch.empty(l2.shape[0], dtype=torch.float32, device=logits.device)
        k.nat.call("sd_twohot_logp_fwd", k.p(l2), k.p(bins), k.p(t), k.p(out), l2.shape[0], NB, k.stream())
        ctx.save_for_backward(l2, bins, t)
        ctx.shape = logits.shape
        return out.view(logits.shape[:-1])

    @staticmethod
    def backward(ctx, g):
        l2, bins, t = ctx.saved_tensors
        dl = torch.empty_like(l2)
        k.nat.call("sd_twohot_logp_bwd", k.p(l2), k.p(bins), k.p(t), k.p(g.contiguous()), k.p(dl), l2.shape[0],
                   l2.shape[1], 0, k.stream())
        return dl.view(ctx.shape), None, None


class RepvalLossFn(torch.autograd.Function):
    """Replay-value loss mean(w * (-logp(ret) - logp(slow))) under the TwoHot value head (dreamer.py:652-658;
    TwoHot.log_prob distributions.py:100-129), w = 1 - is_last. The value head ran on every posterior step: logits
    (B, T, NB), slow / last (B, T); ret (B, T - 1) covers the first T - 1 steps (the reference's [:, :-1] slices are
    read in place). One launch for the row terms, one for their mean (K.device_mean), one backward launch for the
    logits gradient (both log-prob terms; zero on the last step). Targets and weights are detached."""

    @staticmethod
    def forward(ctx, logits, bins, ret, slow, last):
        B, Tl, NB = logits.shape
        Tr = ret.shape[1]
        l2, r, sl, la = logits.contiguous(), ret.contiguous(), slow.contiguous(), last.contiguous()
        rows = torch.empty(B * Tr, dtype=torch.float32, device=logits.device)
        k.nat.call("sd_repval_loss_fwd", k.p(l2), k.p(bins), k.p(r), k.p(sl), k.p(la), k.p(rows), B, Tl, Tr, NB,
                   k.stream())
        ctx.save_for_backward(l2, bins, r, sl, la)
        return k.device_mean(rows)

    @staticmethod
    def backward(ctx, g):
        l2, bins, r, sl, la = ctx.saved_tensors
        B, Tl, NB = l2.shape
        Tr = r.shape[1]
        dl = torch.empty_like(l2)
        gs = g.reshape(1).contiguous()
        k.nat.call("sd_repval_loss_bwd", k.p(l2), k.p(bins), k.p(r), k.p(sl), k.p(la), k.p(gs), 1.0 / (B * Tr),
                   k.p(dl), B, Tl, Tr, NB, k.stream())
        return dl, None, None, None, None


class ImagACLossFn(torch.autograd.Function):
    """Imagined policy and value losses (dreamer.py:623-636, 653-671) and their weighted sum: rows are the H * N
    time-major imagined steps; value logits vl (H*N, NB), logpi / ent (H*N) with gradients; ret (N, H), weight (N, H1),
    val (H1, N) time-major, slow (H, N), scale (device scalar) detached; sp / sv the loss scales. Forward: the row
    terms (sd_imag_ac_loss_fwd) and their means + the weighted total (one sd_loss_terms_fwd); backward: one launch
    from the total's gradient. Returns (total, policy, value, adv): adv (N, H) = (ret - val[:, :H]) / scale; only the
    total carries a gradient."""

    @staticmethod
    def forward(ctx, vl, logpi, ent, bins, ret, slow, weight, val, scale, coef, sp, sv):
        N, H = ret.shape
        H1 = weight.shape[1]
        NB = vl.shape[-1]
        l2 = _flat(vl).contiguous()
        lp, en = logpi.reshape(-1).contiguous(), ent.reshape(-1).contiguous()
        r, sl, w, v = ret.contiguous(), slow.reshape(-1).contiguous(), weight.contiguous(), val.contiguous()
        sc = scale.reshape(1).contiguous()
        rows = torch.empty(2, N * H, dtype=torch.float32, device=vl.device)
        adv = torch.empty(N, H, dtype=torch.float32, device=vl.device)
        k.nat.call("sd_imag_ac_loss_fwd", k.p(l2), k.p(bins), k.p(r), k.p(sl), k.p(w), k.p(v), k.p(sc), k.p(lp),
                   k.p(en), float(coef), N, H, H1, NB, k.p(rows[1]), k.p(rows[0]), k.p(adv), k.stream())
        means = torch.empty(2, dtype=torch.float32, device=vl.device)
        total = torch.empty(1, dtype=torch.float32, device=vl.device)
        k.loss_terms([rows[0], rows[1]], [1.0, 1.0], [sp, sv], means, total)  # policy, value; sp p + sv v
        ctx.save_for_backward(l2, bins, r, sl, w, adv)
        ctx.coef, ctx.sp, ctx.sv, ctx.shapes = float(coef), float(sp), float(sv), (vl.shape, logpi.shape, ent.shape)
        ctx.mark_non_differentiable(means, adv)
        ctx.set_materialize_grads(False)
        return total[0], means[0], means[1], adv

    @staticmethod
    def backward(ctx, g_total, _gp, _gv, _gadv):
        if _gp is not None or _gv is not None:  # (set_materialize_grads(False): unused outputs arrive as None)
            raise RuntimeError("ImagACLossFn: backpropagate the weighted total, not the policy / value loss alone")
        l2, bins, r, sl, w, adv = ctx.saved_tensors
        N, H = r.shape
        H1 = w.shape[1]
        vs, ls, es = ctx.shapes
        if g_total is None:
            return (None,) * 12
        dvl = torch.empty_like(l2)
        dlp = torch.empty(N * H, dtype=torch.float32, device=l2.device)
        den = torch.empty(N * H, dtype=torch.float32, device=l2.device)
        g = g_total.reshape(1).contiguous()
        k.nat.call("sd_imag_ac_loss_bwd", k.p(l2), k.p(bins), k.p(r), k.p(sl), k.p(w), k.p(adv), k.p(g), k.p(g),
                   ctx.sp, ctx.sv, ctx.coef, N, H, H1, l2.shape[1], k.p(dvl), k.p(dlp), k.p(den), k.stream())
        return dvl.view(vs), dlp.view(ls), den.view(es), None, None, None, None, None, None, None, None, None


class BernoulliLogProbFn(torch.autograd.Function):
    """Independent(Bernoulli(logits), 1).log_prob with a single logit (binary head, distributions.py:238)."""

    @staticmethod
    def forward(ctx, logit, value):
        l = logit.reshape(-1).contiguous()
        v = value.reshape(-1).contiguous().float()
        out = torch.empty_like(l)
        k.nat.call("sd_bernoulli_fwd", k.p(l), k.p(v), k.p(out), 0, l.numel(), k.stream())
        ctx.save_for_backward(l, v)
        ctx.shape = logit.shape
        return out.view(logit.shape[:-1])

    @staticmethod
    def backward(ctx, g):
        l, v = ctx.saved_tensors
        dl = torch.empty_like(l)
        k.nat.call("sd_bernoulli_bwd", k.p(l), k.p(v), k.p(g.contiguous()), k.p(dl), l.numel(), k.stream())
        return dl.view(ctx.shape), None


class BNormalLogProbEntFn(torch.autograd.Function):
    """bounded_normal (distributions.py:217-222): Independent(Normal(tanh(mean), std)).log_prob(a), .entropy()."""

    @staticmethod
    def forward(ctx, x, action, min_std, max_std):
        A = action.shape[-1]
        x2 = _flat(x).contiguous()
        a2 = _flat(action).contiguous()
        rows = x2.shape[0]
        lp = torch.empty(rows, dtype=torch.float32, device=x.device)
        ent = torch.empty_like(lp)
        k.nat.call("sd_bnormal_logp_ent_fwd", k.p(x2), k.p(a2), k.p(lp), k.p(ent), rows, A, float(min_std),
                   float(max_std), k.stream())
        ctx.save_for_backward(x2, a2)
        ctx.args = (A, min_std, max_std, x.shape)
        return lp.view(x.shape[:-1]), ent.view(x.shape[:-1])

    @staticmethod
    def backward(ctx, glp, gent):
        x2, a2 = ctx.saved_tensors
        A, mn, mx, shape = ctx.args
        dx = torch.empty_like(x2)
        k.nat.call("sd_bnormal_logp_ent_bwd", k.p(x2), k.p(a2), k.p(None if glp is None else glp.contiguous()),
                   k.p(None if gent is None else gent.contiguous()), k.p(dx), x2.shape[0], A, float(mn), float(mx),
                   k.stream())
        return dx.view(shape), None, None, None


class OneHotLogProbEntFn(torch.autograd.Function):
    """discrete actor OneHotDist (distributions.py:16-36): log_prob(one-hot action), entropy."""

    @staticmethod
    def forward(ctx, logits, action, unimix):
        K = logits.shape[-1]
        l2 = _flat(logits).contiguous()
        a2 = _flat(action).contiguous()
        rows = l2.shape[0]
        lp = torch.empty(rows, dtype=torch.float32, device=logits.device)
        ent = torch.empty_like(lp)
        k.nat.call("sd_onehot_logp_ent_fwd", k.p(l2), k.p(a2), k.p(lp), k.p(ent), rows, K, float(unimix), k.stream())
        ctx.save_for_backward(l2, a2)
        ctx.args = (K, unimix, logits.shape)
        return lp.view(logits.shape[:-1]), ent.view(logits.shape[:-1])

    @staticmethod
    def backward(ctx, glp, gent):
        l2, a2 = ctx.saved_tensors
        K, unimix, shape = ctx.args
        dl = torch.empty_like(l2)
        k.nat.call("sd_onehot_logp_ent_bwd", k.p(l2), k.p(a2), k.p(None if glp is None else glp.contiguous()),
                   k.p(None if gent is None else gent.contiguous()), k.p(dl), l2.shape[0], K, float(unimix),
                   k.stream())
        return dl.view(shape), None, None


class BarlowFn(torch.autograd.Function):
    """R2-Dreamer Barlow loss (dreamer.py:525-532) on x1 (N, E) (with grad) and x2 (N, E) (detached)."""

    @staticmethod
    def forward(ctx, x1, x2, lambd):
        x1, x2 = x1.contiguous(), x2.contiguous()
        Nr, E = x1.shape
        dev = x1.device
        m1, s1 = torch.empty(E, device=dev), torch.empty(E, device=dev)
        m2, s2 = torch.empty(E, device=dev), torch.empty(E, device=dev)
        k.nat.call("sd_colstats", k.p(x1), Nr, E, k.p(m1), k.p(s1), k.stream())
        k.nat.call("sd_colstats", k.p(x2), Nr, E, k.p(m2), k.p(s2), k.stream())
        n1 = torch.empty_like(x1)
        n2 = torch.empty_like(x2)
        k.nat.call("sd_standardize", k.p(x1), k.p(m1), k.p(s1), k.p(n1), Nr, E, 1e-8, k.stream())
        k.nat.call("sd_standardize", k.p(x2), k.p(m2), k.p(s2), k.p(n2), Nr, E, 1e-8, k.stream())
        c = k.mm(n1.t(), n2, alpha=1.0 / Nr)
        nb = 256
        part = torch.empty(2 * nb, device=dev)
        loss = torch.empty(1, device=dev)
        k.nat.call("sd_barlow_loss", k.p(c), E, float(lambd), k.p(part), nb, k.p(loss), k.stream())
        ctx.save_for_backward(x1, m1, s1, n2, c)
        ctx.lambd = lambd
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        x1, m1, s1, n2, c = ctx.saved_tensors
        Nr, E = x1.shape
        dc = torch.empty_like(c)
        gg = g.reshape(1).contiguous()
        k.nat.call("sd_barlow_dc", k.p(c), k.p(gg), k.p(dc), E, float(ctx.lambd), k.stream())
        dn1 = k.mm(n2, dc.t(), alpha=1.0 / Nr)  # c = n1^T n2 / N  ->  dn1 = n2 dc^T / N
        dx1 = torch.empty_like(x1)
        k.nat.call("sd_standardize_bwd", k.p(x1), k.p(m1), k.p(s1), k.p(dn1), k.p(dx1), Nr, E, 1e-8, k.stream())
        return dx1, None, None


class MatmulNTFn(torch.autograd.Function):
    """a (M, K) @ b (N, K)^T with gradients for both operands on the HIP GEMM (DreamerPro's prototype scores,
    dreamer.py:801/811/832, where b is the normalised prototype table: a non-leaf, so its gradient is returned
    through autograd rather than accumulated into a parameter buffer)."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        ctx.save_for_backward(a, b)
        return k.mm(a, b.t())

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        da = k.mm(g, b, fast=True) if ctx.needs_input_grad[0] else None
        db = k.mm(g.t(), a, fast=True) if ctx.needs_input_grad[1] else None
        return da, db


class InfoNCEFn(torch.autograd.Function):
    """InfoNCE loss (dreamer.py:533-542): logits = x1 x2g^T (f32 GEMM), cross entropy against the diagonal; rows of x1
    (n, E) with grad, x2g (Nc, E) detached (all ranks' x2 under data parallel), row r labelled Nc-column r + off.
    Returns the mean over this rank's rows (the DP mean all-reduce of the gradients makes it the global mean)."""

    @staticmethod
    def forward(ctx, x1, x2g, off):
        x1 = x1.contiguous()
        n, nc = x1.shape[0], x2g.shape[0]
        logits = k.mm(x1, x2g.t())
        row = torch.empty(n, dtype=torch.float32, device=x1.device)
        lse = torch.empty(n, dtype=torch.float32, device=x1.device)
        loss = torch.empty(1, dtype=torch.float32, device=x1.device)
        k.nat.call("sd_infonce_fwd", k.p(logits), nc, n, nc, int(off), k.p(row), k.p(lse), k.p(loss), k.stream())
        ctx.save_for_backward(x2g, logits, lse)
        ctx.off = int(off)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        x2g, logits, lse = ctx.saved_tensors
        n, nc = logits.shape
        dl = torch.empty_like(logits)
        gg = g.reshape(1).contiguous()
        k.nat.call("sd_infonce_bwd", k.p(logits), nc, n, nc, ctx.off, k.p(lse), k.p(gg), 1.0 / n, k.p(dl), k.stream())
        return k.mm(dl, x2g, fast=True), None, None

# ------------------------------------------------------------------------------------------------- imagined return
def _mlp_recompute(mods, last, x, fast=False):
    """Pre-activations of [Linear -> RMSNorm -> SiLU] x n + Linear on rows x: ([(pre, rstd)], logits). fast: split-bf16
    contractions (contiguous rows only), else exact f32"""
    saved = []
    for lin, norm in mods:
        pre = k.linear(x, lin.weight, lin.bias, fast=fast)
        x, rstd = k.rmsnorm_fwd(pre, norm.weight)
        saved.append((pre, rstd))
    return saved, k.linear(x, last.weight, last.bias, fast=fast)


def _mlp_input_grad(mods, last, saved, d_logits, rows=None, fast=False):
    """d_logits back to the first layer's pre-norm output (the caller contracts it with the first weight into wherever
    the input gradient goes). rows: (t, N): the saved activations are (H * N, U), this call's rows are step t's."""
    d = k.mm(d_logits, last.weight, fast=fast)
    for i in reversed(range(len(mods))):
        pre, rstd = saved[i]
        if rows is not None:
            t, N = rows
            pre, rstd = pre[t * N:(t + 1) * N], rstd[t * N:(t + 1) * N]
        d = k.rmsnorm_bwd(pre, mods[i][1].weight, rstd, d)
        if i:
            d = k.mm(d, mods[i][0].weight, fast=fast)
    return d


IMAG_RETURN_MARKS = None  # measurement aid (tools/imag_return_bench.py): a list receives (tag, HIP event) per phase


def _mark(tag):
    if IMAG_RETURN_MARKS is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        IMAG_RETURN_MARKS.append((tag, ev))


class ImagineReturnFn(torch.autograd.Function):
    """ret0 (N,): the lambda-return of the frozen actor's imagined rollout from N start states (Dreamer._imagine_tm,
    the reward / continue / value heads' modes, K.lambda_return with boot = value), differentiable in the start state
    only. Forward: the no-grad path itself (fused imagination where the shape admits it, then _heads_returns as the
    update calls it, slow critic included, so that ret is the update's bit for bit); it keeps feats (H1, N, F),
    actions (H1, N, A) and the three (H1, N) head outputs. Backward: every pre-activation is recomputed from the saved
    feats in (H * N)-row GEMMs (no sample is drawn again), the returns' and heads' backward runs on all rows at once,
    and only the state gradient's walk t = H - 1 .. 0 through prior sample -> img_net -> GRU -> dyn_hid -> dyn_in ->
    action sample -> actor is serial. The heads' contractions over all rows (recompute and backward) and the actor's
    recompute run split-bf16, as the forward's heads do; the RSSM's recompute and every serial-step contraction are
    exact f32. No parameter receives a gradient."""

    @staticmethod
    def forward(ctx, post_stoch, post_deter, agent, H1, seed, row_offset, keep):
        r = agent.rssm
        N = post_deter.shape[0]
        if H1 < 2:
            raise ValueError("the imagined return needs a horizon of at least one step (H1 >= 2)")
        mlps = [agent.actor.mlp, agent.reward.mlp, agent.cont.mlp, agent.value.mlp]
        if any(m._symlog_inputs or m.n < 1 for m in mlps):
            raise NotImplementedError("imagined-return backward with symlog-input or layerless actor / heads")
        s = post_stoch.detach().reshape(N, r.flat_stoch).contiguous()
        h = post_deter.detach().contiguous()
        feats, actions = agent._imagine_tm((s, h), H1, seed, row_offset)
        rr = agent._heads_returns(feats)
        if keep is not None:
            keep.update(feats=feats, actions=actions, ret=rr["ret"])
        ctx.save_for_backward(feats, actions, rr["i_rew"], rr["i_val"], rr["i_contl"])
        ctx.agent, ctx.H1, ctx.seed, ctx.row_offset = agent, H1, seed, int(row_offset)
        ctx.stoch_shape = post_stoch.shape
        ctx.set_materialize_grads(False)
        return rr["ret"][:, 0].clone()

    @staticmethod
    def backward(ctx, d_ret0):
        if d_ret0 is None:
            return (None,) * 7
        feats, actions, i_rew, i_val, i_contl = ctx.saved_tensors
        ag, H1, seed, ro = ctx.agent, ctx.H1, ctx.seed, ctx.row_offset
        _mark("begin")
        d_st, d_de = _imag_heads_grad(ag, feats, i_rew, i_val, i_contl, d_ret0, H1)
        _mark("heads")
        rec = _imag_recompute(ag, feats, actions, H1)
        _mark("recompute")
        if imag_walk_is_fused(ag, rec):
            _imag_walk_fused(ag, rec, d_st, d_de, seed, ro)
            _mark("walk")
        else:
            _imag_walk_per_op(ag, rec, d_st, d_de, seed, ro)
        return d_st[0].reshape(ctx.stoch_shape), d_de[0], None, None, None, None, None


def _imag_heads_grad(ag, feats, i_rew, i_val, i_contl, d_ret0, H1):
    """Batched over all rows: the returns' backward, then the heads' (rows of steps 1 .. H; step 0 has none) ->
    d_st (H1, N, SK), d_de (H1, N, D): the gradient that reaches every step's feat from outside the rollout."""
    r = ag.rssm
    H, N, F = H1 - 1, feats.shape[1], feats.shape[2]
    SK, M = r._stoch * r._discrete, H * N
    dev, f32 = feats.device, torch.float32
    d_ret = torch.zeros(N, H, dtype=f32, device=dev)
    d_ret[:, 0] = d_ret0
    d_rew, d_val, d_cl = k.lambda_return_bwd(d_ret, i_rew.t(), i_val.t(), i_contl.t(), 1 - 1 / ag.horizon, ag.lamb,
                                             time_major=True)
    d_feat = torch.empty(H1, N, F, dtype=f32, device=dev)
    d_feat[0].zero_()
    xh = feats[1:].reshape(M, F)
    dfh = d_feat[1:].view(M, F)
    for i, (head, bins, d_out) in enumerate(((ag.reward, ag.rbins, d_rew), (ag.cont, None, d_cl),
                                             (ag.value, ag.vbins, d_val))):
        saved, logits = _mlp_recompute(head.mlp._mods, head.last, xh, fast=True)
        d_out = d_out[1:].reshape(M)
        d_logits = d_out.view(M, 1) if bins is None else k.twohot_mode_bwd(logits, bins, d_out)
        d0 = _mlp_input_grad(head.mlp._mods, head.last, saved, d_logits, fast=True)
        k.gemm(d0, head.mlp._mods[0][0].weight, dfh, beta=1.0 if i else 0.0, fast=True)
        del saved, logits
    return d_feat[..., :SK].contiguous(), d_feat[..., SK:].contiguous()


def _imag_recompute(ag, feats, actions, H1):
    """Batched: every pre-activation of steps 0 .. H - 1 from the saved feats and actions (rows t * N + n), as a dict
    the two walks read."""
    r = ag.rssm
    P = r._p()
    H, N, F = H1 - 1, feats.shape[1], feats.shape[2]
    S, Kd, D, U, G, A = r._stoch, r._discrete, r._deter, r._hidden, r._blocks, ag.act_dim
    SK, Dg, M = S * Kd, D // G, H * N
    e = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=feats.device)  # noqa: E731
    xh = feats[1:].reshape(M, F)
    xa = feats[:H].reshape(M, F)
    h_in = xa[:, SK:].contiguous()
    a_n = k.action_norm(actions[:H].reshape(M, A))
    xcat = e(M, 3 * U)
    x0p, x1p, x2p = k.linear(h_in, P["W0"], P["b0"]), k.linear(xa[:, :SK], P["W1"], P["b1"]), \
        k.linear(a_n, P["W2"], P["b2"])
    _, r0 = k.rmsnorm_fwd(x0p, P["n0"], y=xcat[:, :U])
    _, r1 = k.rmsnorm_fwd(x1p, P["n1"], y=xcat[:, U:2 * U])
    _, r2 = k.rmsnorm_fwd(x2p, P["n2"], y=xcat[:, 2 * U:])
    hp = k.mm(xcat, P["Wsh"].t(), bias=P["bh"])
    k.gemm(h_in.view(M, G, Dg).permute(1, 0, 2), P["Wbd"].transpose(1, 2), hp.view(M, G, Dg).permute(1, 0, 2),
           beta=1.0)
    hh, rh = k.rmsnorm_fwd(hp, P["nh"])
    gates = e(M, 3 * D)
    k.gemm(hh.view(M, G, Dg).permute(1, 0, 2), P["Wg"].transpose(1, 2), gates.view(M, G, 3 * Dg).permute(1, 0, 2),
           bias=P["bg"].view(G, 3 * Dg))
    del xcat, hh
    img_mods, img_last = r._img_mods()
    img_saved, plogit = _mlp_recompute(img_mods, img_last, xh[:, SK:])
    act_mods, act_last = ag.actor.mlp._mods, ag.actor.last
    act_saved, alogit = _mlp_recompute(act_mods, act_last, xa, fast=True)
    return dict(feats=feats, actions=actions, H=H, N=N, h_in=h_in, x0p=x0p, x1p=x1p, x2p=x2p, r0=r0, r1=r1, r2=r2,
                hp=hp, rh=rh, gates=gates, img_saved=img_saved, plogit=plogit, act_saved=act_saved, alogit=alogit)


def _imag_walk_per_op(ag, rec, d_st, d_de, seed, ro):
    """The serial walk as per-op launches: d_feat[t + 1] = (d_st[t + 1], d_de[t + 1]) is complete; add step t's part
    into d_feat[t], t = H - 1 .. 0."""
    from .rssm import STREAM_ACT, STREAM_IMG
    r = ag.rssm
    P = r._p()
    H, N = rec["H"], rec["N"]
    S, Kd, D, U, G, A = r._stoch, r._discrete, r._deter, r._hidden, r._blocks, ag.act_dim
    SK, Dg = S * Kd, D // G
    actions, h_in, gates, hp, rh = rec["actions"], rec["h_in"], rec["gates"], rec["hp"], rec["rh"]
    x0p, x1p, x2p, r0, r1, r2 = (rec[n] for n in ("x0p", "x1p", "x2p", "r0", "r1", "r2"))
    img_saved, plogit, act_saved, alogit = rec["img_saved"], rec["plogit"], rec["act_saved"], rec["alogit"]
    img_mods, img_last = r._img_mods()
    act_mods, act_last = ag.actor.mlp._mods, ag.actor.last
    Wi0, Wa0 = img_mods[0][0].weight, act_mods[0][0].weight
    dist = ag.config.actor.dist
    e = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=d_st.device)  # noqa: E731
    step = lambda x, t: x[t * N:(t + 1) * N]  # noqa: E731
    for t in reversed(range(H)):
        dl = k.onehot_sample_bwd(step(plogit, t), d_st[t + 1], Kd, r._unimix_ratio, seed, STREAM_IMG, t, ro * S)
        k.gemm(_mlp_input_grad(img_mods, img_last, img_saved, dl, (t, N)), Wi0, d_de[t + 1], beta=1.0)
        d_gates, _ = k.gru_bwd(step(gates, t), step(h_in, t), d_de[t + 1], G, dh=d_de[t], accumulate_dh=True)
        d_hh = e(N, D)
        k.gemm(d_gates.view(N, G, 3 * Dg).permute(1, 0, 2), P["Wg"], d_hh.view(N, G, Dg).permute(1, 0, 2))
        d_hp = k.rmsnorm_bwd(step(hp, t), P["nh"], step(rh, t), d_hh)
        d_xcat = k.mm(d_hp, P["Wsh"])
        k.gemm(d_hp.view(N, G, Dg).permute(1, 0, 2), P["Wbd"], d_de[t].view(N, G, Dg).permute(1, 0, 2), beta=1.0)
        d_x0p = k.rmsnorm_bwd(step(x0p, t), P["n0"], step(r0, t), d_xcat[:, :U])
        k.gemm(d_x0p, P["W0"], d_de[t], beta=1.0)
        d_x1p = k.rmsnorm_bwd(step(x1p, t), P["n1"], step(r1, t), d_xcat[:, U:2 * U])
        k.gemm(d_x1p, P["W1"], d_st[t], beta=1.0)
        d_x2p = k.rmsnorm_bwd(step(x2p, t), P["n2"], step(r2, t), d_xcat[:, 2 * U:])
        d_an = k.mm(d_x2p, P["W2"])
        if ag.act_discrete:  # the normalisation is the identity on a one-hot
            d_al = k.onehot_sample_bwd(step(alogit, t), d_an, A, float(dist.unimix_ratio), seed, STREAM_ACT, t, ro)
        else:
            d_al = k.bnormal_sample_bwd(d_an, step(alogit, t), actions[t], float(dist.min_std),
                                        float(dist.max_std), seed, STREAM_ACT, t, ro)
        d_a0 = _mlp_input_grad(act_mods, act_last, act_saved, d_al, (t, N))
        k.gemm(d_a0, Wa0[:, :SK], d_st[t], beta=1.0)
        k.gemm(d_a0, Wa0[:, SK:], d_de[t], beta=1.0)
        _mark("step")


def _imag_bwd_desc(ag, rec, d_st, d_de, seed, ro):
    """sd_imagine_bwd's descriptor over the recomputed activations (d_st / d_de may be None: the shape questions only);
    -> (descriptor, the tensors it points to that nothing else holds)"""
    import ctypes
    from .rssm import STREAM_ACT, STREAM_IMG
    r, a = ag.rssm, ag.actor
    P = r._p()
    d = k.nat.ImagineBwdDesc()
    d.N, d.H1, d.D, d.U, d.SK, d.Kd, d.G, d.A = rec["N"], rec["H"] + 1, r._deter, r._hidden, r.flat_stoch, \
        r._discrete, r._blocks, ag.act_dim
    d.act_discrete, d.actor_layers, d.img_layers = int(ag.act_discrete), a.mlp.n, r._img_layers
    dist = ag.config.actor.dist
    d.eps, d.unimix = k.EPS, r._unimix_ratio
    if ag.act_discrete:
        d.act_unimix = float(dist.unimix_ratio)
    else:
        d.min_std, d.max_std = float(dist.min_std), float(dist.max_std)
    d.seed, d.seed_ptr = k.seed_args(seed)
    d.stream_img, d.stream_act, d.row_offset = STREAM_IMG, STREAM_ACT, int(ro)
    hold = []
    for i, (lin, norm) in enumerate(a.mlp._mods):
        d.Wa[i], d.na[i] = lin.weight.data_ptr(), norm.weight.data_ptr()
        pre, rstd = rec["act_saved"][i]
        d.act_pre[i], d.act_rstd[i] = pre.data_ptr(), rstd.data_ptr()
    wo = a.last.weight.contiguous()
    hold.append(wo)
    d.Wao = wo.data_ptr()
    for n in ("W0", "n0", "W1", "n1", "W2", "n2", "Wh", "nh", "Wg"):
        setattr(d, n, P[n].data_ptr())
    mods, last = r._img_mods()
    for i, (lin, norm) in enumerate(mods):
        d.Wi[i], d.ni[i] = lin.weight.data_ptr(), norm.weight.data_ptr()
        pre, rstd = rec["img_saved"][i]
        d.img_pre[i], d.img_rstd[i] = pre.data_ptr(), rstd.data_ptr()
    d.Wl = last.weight.data_ptr()
    d.feats, d.actions = rec["feats"].data_ptr(), rec["actions"].data_ptr()
    for n in ("x0p", "x1p", "x2p", "r0", "r1", "r2", "hp", "rh", "gates", "plogit", "alogit"):
        assert rec[n].is_contiguous(), n
        setattr(d, n, rec[n].data_ptr())
    if d_st is not None:
        assert d_st.is_contiguous() and d_de.is_contiguous()
        d.d_stoch, d.d_deter = d_st.data_ptr(), d_de.data_ptr()
    return d, hold, ctypes.addressof(d)


def imag_walk_is_fused(ag, rec):
    """The one route decision of the serial walk: the fused imagination's gate and sd_imagine_bwd's own."""
    if not ag._fused_imag_ok():
        return False
    _d, _hold, addr = _imag_bwd_desc(ag, rec, None, None, 0, 0)
    return k.nat.fns["sd_imagine_bwd_ok"](addr) == 1


def _imag_walk_fused(ag, rec, d_st, d_de, seed, ro, chunks=None, work=None):
    """The serial walk as sd_imagine_bwd (csrc/imgbwd.hip), 7 launches per step. chunks: step boundaries
    [0, t1, ..., H], walked last chunk first (one ABI call each); work: a workspace to reuse."""
    d, hold, addr = _imag_bwd_desc(ag, rec, d_st, d_de, seed, ro)
    nwork = k.nat.fns["sd_imagine_bwd_work_floats"](addr)
    if nwork < 0:
        raise k.nat.NativeError(f"sd_imagine_bwd_work_floats failed with status {nwork}")
    if work is None:
        work = torch.empty(nwork, dtype=torch.float32, device=d_st.device)
    assert work.numel() >= nwork
    d.work = work.data_ptr()
    bounds = list(chunks) if chunks else [0, rec["H"]]
    for t0, t1 in reversed(list(zip(bounds[:-1], bounds[1:]))):
        d.t_begin, d.t_end = int(t0), int(t1)
        k.nat.call("sd_imagine_bwd", addr, k.stream())
    return work
