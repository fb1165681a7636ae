"""Text-conditioned encoder kernels on the MI355X against float64 torch: the FiLM stage (forward and backward, every
fused forward kernel the plain stage selects), its identity with the plain stage at gamma = 1 / beta = 0, the text
gate, the text pooling, run-to-run determinism of the per-context-row reductions, and the modules end to end."""
import types

import pytest
import torch
import torch.nn.functional as F

import mm_ref
from golden_io import sample_idx
from oracle import ref_cpu as R
from test_gpu_ops import _g, close

pytestmark = pytest.mark.gpu
DEV = "cuda"

STAGES = [(4, 32, 64), (32, 48, 32), (48, 64, 16), (64, 64, 8)]


def _stage_inputs(ci, co, hw, rows, ipc):
    nb = rows * ipc
    x = torch.rand(nb, hw, hw, ci, generator=_g(ci)) - 0.5
    w = torch.randn(co, ci, 5, 5, generator=_g(co)) / (ci * 25) ** 0.5
    b = 0.1 * torch.randn(co, generator=_g(1))
    nw = 1 + 0.1 * torch.randn(co, generator=_g(2))
    gamma = 1 + 0.5 * torch.randn(rows, co, generator=_g(4))  # every context row its own modulation
    beta = 0.5 * torch.randn(rows, co, generator=_g(5))
    return x, w, b, nw, gamma, beta


def _film_ref(x, w, b, nw, gamma, beta, ipc, nchw):
    """conv_same -> max_pool2d -> rms2d -> gamma x + beta -> silu in float64; returns (y, leaves)"""
    leaves = [t.double().clone().requires_grad_() for t in (x, w, b, nw, gamma, beta)]
    xr, wr, br, nwr, gr, ber = leaves
    y = R.rms2d(F.max_pool2d(R.conv_same(xr.permute(0, 3, 1, 2), wr, br), 2, 2), nwr)
    ge = gr.repeat_interleave(ipc, 0)[:, :, None, None]
    be = ber.repeat_interleave(ipc, 0)[:, :, None, None]
    y = F.silu(ge * y + be)
    y = y.reshape(y.shape[0], -1) if nchw else y.permute(0, 2, 3, 1)
    return y, leaves


def _film_dev(x, w, b, nw, gamma, beta, nchw, need_dx=True):
    from sdreamer import ops
    xd = x.to(DEV).requires_grad_(need_dx)
    wd = w.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_()
    rest = [t.to(DEV).requires_grad_() for t in (b, nw, gamma, beta)]
    out = ops.FilmConvPoolNormFn.apply(xd, wd, *rest, nchw)
    return out, [xd, wd] + rest


def _check_stage(ci, co, hw, rows, ipc, nchw, need_dx=True):
    x, w, b, nw, gamma, beta = _stage_inputs(ci, co, hw, rows, ipc)
    ref, (xr, wr, br, nwr, gr, ber) = _film_ref(x, w, b, nw, gamma, beta, ipc, nchw)
    dy = torch.randn(ref.shape, generator=_g(3))
    ref.backward(dy.double())
    out, (xd, wd, bd, nwd, gd, bed) = _film_dev(x, w, b, nw, gamma, beta, nchw, need_dx)
    close(out, ref, 2e-5, "fwd")
    out.backward(dy.to(DEV))
    if need_dx:
        close(xd.grad, xr.grad, 5e-5, "dx")
    close(wd.grad.permute(0, 3, 1, 2), wr.grad, 5e-5, "dw")
    close(bd.grad, br.grad, 5e-5, "db")
    close(nwd.grad, nwr.grad, 5e-5, "dnw")
    close(gd.grad, gr.grad, 5e-5, "dgamma")
    close(bed.grad, ber.grad, 5e-5, "dbeta")


@pytest.mark.parametrize("rows,ipc", [(2, 3), (3, 1)])
@pytest.mark.parametrize("ci,co,hw", STAGES)
def test_film_stage_matches_float64(ci, co, hw, rows, ipc):
    """B.T = 2.3: at 8 x 8 a 128-pixel tile holds two images, so the second tile straddles context rows 0 and 1 and
    three tiles leave no padding; B.T = 3.1 is the act shape (every image its own row)."""
    _check_stage(ci, co, hw, rows, ipc, nchw=(hw == 8))


def test_film_last_stage_nhwc():
    _check_stage(64, 64, 8, 2, 3, nchw=False)


def test_film_first_stage_compact_backward():
    """no input gradient: the pooled-resolution backward (sd_pool_rms_bwd_compact_film) feeds the bwd-weight kernel"""
    _check_stage(4, 32, 64, 2, 3, nchw=False, need_dx=False)


@pytest.mark.parametrize("conv6", ["1", ""])
@pytest.mark.parametrize("ci,co,hw", STAGES[1:3])
def test_film_stage_conv6_on_off(ci, co, hw, conv6, monkeypatch):
    from sdreamer import kernels as K
    monkeypatch.setattr(K, "CONV6", conv6)
    _check_stage(ci, co, hw, 2, 3, nchw=False)


def test_film_two_launch_forward_matches_fused(monkeypatch):
    from sdreamer import kernels as K
    x, w, b, nw, gamma, beta = [t.to(DEV) for t in _stage_inputs(64, 64, 8, 2, 3)]
    w = w.permute(0, 2, 3, 1).contiguous()
    monkeypatch.setattr(K, "CONV6", "")
    fused = K.conv2d_fwd_pool(x, w, b, nw, nchw_flat=True, film=(gamma, beta))
    assert fused is not None, "shape should take the fused kernel"
    two = K.pool_rms_fwd(K.conv2d_fwd(x, w, b), nw, nchw_flat=True, film=(gamma, beta))
    assert torch.equal(fused[1], two[1]) and torch.equal(fused[2], two[2])  # pooled, amax: same k order
    close(fused[0], two[0], 1e-6, "y")
    close(fused[3], two[3], 1e-6, "rstd")


@pytest.mark.parametrize("ci,co,hw", STAGES)
def test_film_identity_equals_plain_stage_bitwise(ci, co, hw):
    """gamma = 1, beta = 0: the FiLM path is ConvPoolNormFn bit for bit (outputs, saved tensors, every gradient)"""
    from sdreamer import ops
    rows, ipc = 2, 3
    x, w, b, nw, _, _ = _stage_inputs(ci, co, hw, rows, ipc)
    nchw = hw == 8
    dy = None
    got = {}
    for film in (False, True):
        xd = x.to(DEV).requires_grad_(ci != 4)
        wd = w.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_()
        bd, nwd = b.to(DEV).requires_grad_(), nw.to(DEV).requires_grad_()
        if film:
            gam = torch.ones(rows, co, device=DEV).requires_grad_()
            bet = torch.zeros(rows, co, device=DEV).requires_grad_()
            out = ops.FilmConvPoolNormFn.apply(xd, wd, bd, nwd, gam, bet, nchw)
        else:
            out = ops.ConvPoolNormFn.apply(xd, wd, bd, nwd, nchw)
        saved = out.grad_fn.saved_tensors
        dy = torch.randn(out.shape, generator=_g(3)).to(DEV) if dy is None else dy
        out.backward(dy)
        got[film] = dict(y=out.detach(), pooled=saved[4], amax=saved[5], rstd=saved[6], dx=xd.grad, dw=wd.grad,
                         db=bd.grad, dnw=nwd.grad)
    for k in got[False]:
        a, f = got[False][k], got[True][k]
        assert (a is None) == (f is None), k
        if a is not None:
            assert torch.equal(a, f), k


def _gate_ref(v, a, tp, T):
    leaves = [t.double().clone().requires_grad_() for t in (v, a, tp)]
    vr, ar, tpr = leaves
    g = torch.sigmoid(ar)
    te = tpr.repeat_interleave(T, 0)
    return (1 - g) * vr + g * te, g, leaves


@pytest.mark.parametrize("B,T,E", [(2, 3, 1024), (3, 5, 80)])
def test_text_gate_matches_float64(B, T, E):
    from sdreamer import kernels as K
    from sdreamer import ops
    v = torch.randn(B * T, E, generator=_g(1))
    a = 2 * torch.randn(B * T, E, generator=_g(2))
    tp = torch.randn(B, E, generator=_g(3))
    d = torch.randn(B * T, E, generator=_g(4))
    ref, gref, (vr, ar, tpr) = _gate_ref(v, a, tp, T)
    ref.backward(d.double())
    vd, ad, tpd = [t.to(DEV).requires_grad_() for t in (v, a, tp)]
    out, g = ops.text_gate(vd, ad, tpd, T)
    close(out, ref, 1e-6, "out")
    close(g, gref, 1e-6, "g")
    out.backward(d.to(DEV))
    close(vd.grad, vr.grad, 1e-6, "dv")
    close(ad.grad, ar.grad, 1e-6, "da")
    close(tpd.grad, tpr.grad, 1e-5, "dtp")
    # the diagnostics, resolved like every other metric of the update (no host sync until read)
    vec = K.metric_vector([K.Stat(g, K.STAT_MEAN), K.Stat(g, K.STAT_STD)])
    close(vec[0], gref.mean(), 1e-6, "gate mean")
    close(vec[1], gref.std(), 1e-6, "gate std (unbiased)")


@pytest.mark.parametrize("ntok", [1, 7, 77])
def test_text_pool_matches_float64(ntok):
    from sdreamer import kernels as K
    f = torch.randn(ntok, 512, generator=_g(ntok))
    w = torch.randn(1, 512, generator=_g(1)) / 512 ** 0.5
    b = torch.tensor([0.3])
    fd, wd_, bd = f.double(), w.double(), b.double()
    p = torch.softmax(fd @ wd_.t() + bd, 0)
    ref = (fd * p).sum(0, keepdim=True)
    out = K.text_pool(f.to(DEV), w.to(DEV), b.to(DEV))
    close(out, ref, 1e-6, "pooled")
    two = K.text_pool(torch.stack([f, f.flip(0)]).to(DEV), w.to(DEV), b.to(DEV))  # token order does not matter
    close(two[0:1], ref, 1e-6, "pooled, batched")
    close(two[1:2], ref, 1e-6, "pooled, batched, reversed tokens")


@pytest.mark.parametrize("T,E", [(3, 80), (1, 64)])
def test_rowbias_silu_matches_float64(T, E):
    from sdreamer import ops
    B = 3
    x = torch.randn(B * T, E, generator=_g(1))
    u = torch.randn(B, E, generator=_g(2))
    d = torch.randn(B * T, E, generator=_g(3))
    xr, ur = x.double().requires_grad_(), u.double().requires_grad_()
    ref = F.silu(xr + ur.repeat_interleave(T, 0))
    ref.backward(d.double())
    xd, ud = x.to(DEV).requires_grad_(), u.to(DEV).requires_grad_()
    out = ops.rowbias_silu(xd, ud, T)
    close(out, ref, 1e-6, "fwd")
    out.backward(d.to(DEV))
    close(xd.grad, xr.grad, 1e-6, "dx")
    close(ud.grad, ur.grad, 1e-5, "du")
    plain = ops.rowbias_silu(x.to(DEV))
    close(plain, F.silu(x.double()), 1e-6, "plain silu")


def test_reductions_are_deterministic():
    """dgamma, dbeta, dnw and dtp twice on the same inputs: bit-equal (fixed-order sums, no atomics)"""
    from sdreamer import ops
    x, w, b, nw, gamma, beta = _stage_inputs(32, 48, 32, 2, 3)
    dy = torch.randn(6, 16, 16, 48, generator=_g(3)).to(DEV)
    runs = []
    for _ in range(2):
        out, (xd, wd, bd, nwd, gd, bed) = _film_dev(x, w, b, nw, gamma, beta, False)
        out.backward(dy)
        runs.append((gd.grad, bed.grad, nwd.grad, xd.grad))
    for a, c in zip(*runs):
        assert torch.equal(a, c)
    v, a_, tp = torch.randn(6, 1024, generator=_g(1)), torch.randn(6, 1024, generator=_g(2)), torch.randn(2, 1024)
    d = torch.randn(6, 1024, generator=_g(4)).to(DEV)
    dtps = []
    for _ in range(2):
        vd, ad, tpd = [t.to(DEV).requires_grad_() for t in (v, a_, tp)]
        ops.text_gate(vd, ad, tpd, 3)[0].backward(d)
        dtps.append(tpd.grad)
    assert torch.equal(*dtps)


def test_mlp_projector_uses_machine_epsilon():
    """nn.RMSNorm(eps=None): rows small enough that 1e-4 and 1.19e-7 give different answers"""
    from sdreamer.multimodal import MLPProjector
    torch.manual_seed(0)
    prj = MLPProjector(96, 64).to(DEV)
    x = 1e-3 * torch.randn(8, 96, generator=_g(1))
    xr = x.double().requires_grad_()
    w1, nw, w2 = [p.detach().double().cpu().requires_grad_() for p in (prj.fc1.weight, prj.norm.weight,
                                                                       prj.fc2.weight)]
    h = F.linear(xr, w1)
    ref = F.linear(F.silu(F.rms_norm(h, (64,), nw, float(torch.finfo(torch.float32).eps))), w2)
    wrong = F.linear(F.silu(F.rms_norm(h, (64,), nw, 1e-4)), w2)
    d = torch.randn(8, 64, generator=_g(2))
    ref.backward(d.double())
    xd = x.to(DEV).requires_grad_()
    out = prj(xd)
    close(out, ref, 2e-5, "fwd")
    assert (out.double().cpu() - wrong).abs().max().item() > 0.05 * ref.abs().max().item()
    out.backward(d.to(DEV))
    # gradient contractions run split-bf16 (~1e-5 relative)
    close(xd.grad, xr.grad, 1e-4, "dx")
    close(prj.fc1.weight.grad, w1.grad, 1e-4, "dfc1")
    close(prj.norm.weight.grad, nw.grad, 1e-4, "dnorm")
    close(prj.fc2.weight.grad, w2.grad, 1e-4, "dfc2")


def _cnn_cfg():
    return types.SimpleNamespace(depth=16, mults=[2, 3, 4, 4], kernel_size=5, norm=True, act="SiLU")


def _dense_(module, seed):
    """dense deterministic values everywhere, so the zero-initialised FiLM and gate layers are exercised"""
    g = _g(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("norms.0.weight") or ".norms." in name or name.endswith("norm.weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            elif p.dim() > 1:
                fan_in = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) / fan_in ** 0.5)
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))


def _encoder_ref(sd, feats, img, B, T, gate):
    """text pooling -> FiLM encoder -> gate in float64 (tests/mm_ref.py) from the reference-layout state dict"""
    P = mm_ref.f64_params(sd)
    visual, gated, g, ctx = mm_ref.encoder_ref(P, feats, img, B, T, "mm", gate)
    return visual, gated, g, P, ctx.expand(B, -1)


@pytest.mark.parametrize("B,T", [(2, 3), (3, 1)])
def test_multimodal_encoder_matches_float64(B, T):
    """MultimodalEncoder end to end (text pooling -> FiLM encoder -> gate), forward and every parameter gradient,
    against the float64 restatement; the frozen text front end receives no gradient."""
    from sdreamer import kernels as K
    from sdreamer.multimodal import MultimodalEncoder
    enc = MultimodalEncoder(_cnn_cfg(), (64, 64, 3), seed_base=3)
    _dense_(enc, 7)
    enc = enc.to(DEV).train()
    feats = [torch.randn(n, 512, generator=_g(n)) for n in (7, 12)]
    enc.set_text_features(["a walker", "a runner"], feats)
    enc.set_task_name("walker_walk")
    img = torch.rand(B, T, 64, 64, 3, generator=_g(9)) if T > 1 else torch.rand(B, 64, 64, 3, generator=_g(9))
    visual, gated = enc({"image": img.to(DEV)})
    idx = enc._cached_index
    rv, rg, g, P, ctx = _encoder_ref(enc.state_dict(), feats[idx], img, B, T, gate=True)
    shape = (B, T, -1) if T > 1 else (B, -1)
    close(enc._ctx, ctx, 1e-5, "text context")
    close(visual, rv.reshape(*shape), 1e-4, "visual_embed")
    close(gated, rg.reshape(*shape), 1e-4, "rssm_embed")
    vec = K.metric_vector(list(enc.gate_metrics().values()))
    close(vec[0], g.mean(), 1e-4, "gate mean")
    close(vec[1], g.std(), 1e-4, "gate std")
    d1, d2 = torch.randn(rv.shape, generator=_g(1)), torch.randn(rv.shape, generator=_g(2))
    ((rv * d1.double()).sum() + (rg * d2.double()).sum()).backward()
    ((visual.reshape(rv.shape) * d1.to(DEV)).sum() + (gated.reshape(rv.shape) * d2.to(DEV)).sum()).backward()
    sd_grads = {}
    for name, p in enc.named_parameters():
        if name.startswith("text_context_encoder."):
            assert p.grad is None, name
            continue
        gr = p.grad
        if ".convs." in name and name.endswith("weight"):
            gr = gr.permute(0, 3, 1, 2)
        sd_grads[name] = gr
    for name, gr in sd_grads.items():
        ref = P[name].grad
        # every gradient contraction runs split-bf16, ~1e-5 of its output scale each; the first conv's
        # weight gradient is behind ten of them (gate: 3, text_proj / FiLM: 2, three conv bwd-data, its own
        # bwd-weight), each error carried on by factors of order one: 10 x 1e-5 with a factor 5 for that growth
        close(gr, ref, 5e-4, name)
        assert ref.abs().max().item() > 0, name
    # a second forward inside the resample interval reuses the context buffer (same address: graphs can read it)
    ptr = enc._ctx.data_ptr()
    enc({"image": img.to(DEV)})
    assert enc._ctx.data_ptr() == ptr and enc._forward_count == 2
    enc.text_context(B, DEV, force_index=1 - idx)  # a text switch rewrites the buffer in place
    assert enc._ctx.data_ptr() == ptr and enc._cached_index == 1 - idx


def test_gate_only_and_film_only_forward():
    from sdreamer.multimodal import GateOnlyEncoder, MultimodalEncoder
    B, T = 2, 3
    feats = [torch.randn(7, 512, generator=_g(7))]
    img = torch.rand(B, T, 64, 64, 3, generator=_g(9))
    film = MultimodalEncoder(_cnn_cfg(), (64, 64, 3), use_text_gate=False)
    _dense_(film, 7)
    film = film.to(DEV)
    film.set_text_features(["t"], feats)
    out = film({"image": img.to(DEV)})
    rv, _, _, _, _ = _encoder_ref(film.state_dict(), feats[0], img, B, T, gate=False)
    close(out, rv.reshape(B, T, -1), 1e-4, "film-only visual_embed")
    go = GateOnlyEncoder(_cnn_cfg(), (64, 64, 3))
    _dense_(go, 8)
    go = go.to(DEV)
    go.set_text_features(["t"], feats)
    visual, gated = go({"image": img.to(DEV)})
    x = torch.nn.functional.pad(img.reshape(B * T, 64, 64, 3) - 0.5, (0, 1)).to(DEV)
    assert torch.equal(visual, go.conv_encoder(x).reshape(B, T, -1)), "gate-only visual_embed is the ConvEncoder's"
    gate2, g = go.text_gate(visual.reshape(B * T, -1), go._ctx)
    assert torch.equal(gated.reshape(B * T, -1), gate2)
    assert 0 < g.min().item() and g.max().item() < 1


def _allclose(a, b, rtol, atol, what):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double()
    err = (a - b).abs()
    worst = (err / (atol + rtol * b.abs())).max().item()
    print(f"{what}: worst bound ratio {worst:.3f}")
    assert worst <= 1, f"{what}: {worst} x the bound"


@pytest.mark.parametrize("name", sorted(mm_ref.CASES))
def test_encoder_matches_reference_fixture(name):
    """The modules against the reference's own outputs (tests/golden/encoder_mm_*.npz): embeds at the update test's
    1e-4 / 1e-5, gate mean / std at 1e-4 relative, every trainable tensor's gradient at the _cal_grad test's bounds
    (sampled elements within 2e-3 relative + 1e-4 of the largest sampled |g|, norms within 2e-4), the text front end
    without gradient; then the act shape in eval mode (first text)."""
    from sdreamer import kernels as K
    from sdreamer.multimodal import GateOnlyEncoder, MultimodalEncoder
    kind, gate = mm_ref.CASES[name]
    z = mm_ref.load_fixture(name)
    cls = MultimodalEncoder if kind == "mm" else GateOnlyEncoder
    enc = cls(_cnn_cfg(), (64, 64, 3), use_text_gate=gate)
    enc.load_state_dict(mm_ref.fixture_params(enc.state_dict()))
    enc = enc.to(DEV).train()
    enc.set_text_features([str(t) for t in z["texts"]], [z["feat_0"], z["feat_1"]])
    enc.set_task_name("walker_walk")
    img = (torch.from_numpy(z["image"]).float() / 255.0).to(DEV)
    B, T = img.shape[:2]
    ctx = enc.text_context(B, DEV, force_index=int(z["train_text"]))  # the text the reference's forward drew
    _allclose(ctx[0], z["ctx"], 1e-4, 1e-5, "text context")
    res = enc({"image": img}, reuse_text_context=ctx)
    visual, gated = res if gate else (res, None)
    _allclose(visual, z["visual_embed"], 1e-4, 1e-5, "visual_embed")
    loss = (visual * torch.from_numpy(z["d_visual"]).to(DEV)).sum()
    if gate:
        _allclose(gated, z["rssm_embed"], 1e-4, 1e-5, "rssm_embed")
        vec = K.metric_vector(list(enc.gate_metrics().values()))
        _allclose(vec[0], z["gate_mean"], 1e-4, 0.0, "gate mean")
        _allclose(vec[1], z["gate_std"], 1e-4, 0.0, "gate std")
        loss = loss + (gated * torch.from_numpy(z["d_rssm"]).to(DEV)).sum()
    loss.backward()
    worst_e = worst_n = 0.0
    for k, p in enc.named_parameters():
        key = "encoder." + k
        if k.startswith("text_context_encoder."):
            assert p.grad is None and f"gradnone__{key}" in z.files, key
            continue
        gr = p.grad
        if gr.dim() == 4:  # conv weights: internal (Co, kh, kw, Ci) -> reference (Co, Ci, kh, kw)
            gr = gr.permute(0, 3, 1, 2)
        gr = gr.reshape(-1).double().cpu().numpy()
        ref = z[f"grad__{key}"].astype("float64")
        got = gr[sample_idx(key, gr.size)]
        ratio = (abs(got - ref) / (2e-3 * abs(ref) + 1e-4 * abs(ref).max())).max()
        nratio = abs((gr ** 2).sum() ** 0.5 / float(z[f"gradnorm__{key}"]) - 1) / 2e-4
        worst_e, worst_n = max(worst_e, ratio), max(worst_n, nratio)
        assert ratio <= 1 and nratio <= 1, f"{key}: elements {ratio} x, norm {nratio} x the bound"
    print(f"gradients: worst element bound ratio {worst_e:.3f}, worst norm bound ratio {worst_n:.3f}")
    enc.eval()
    img1 = (torch.from_numpy(z["act_image"]).float() / 255.0).to(DEV)
    with torch.no_grad():
        res = enc({"image": img1})
    visual, gated = res if gate else (res, None)
    assert enc._cached_index == 0
    _allclose(visual, z["act_visual_embed"], 1e-4, 1e-5, "act visual_embed")
    if gate:
        _allclose(gated, z["act_rssm_embed"], 1e-4, 1e-5, "act rssm_embed")
