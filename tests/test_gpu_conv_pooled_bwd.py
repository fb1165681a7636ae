"""The split-bf16 backward contractions of a pooled encoder stage from the pooled gradient (sd_conv2d_wgrad_bf16x3_pooled,
sd_conv2d_dgrad_direct_pooled; ops.ConvPoolNormFn / FilmConvPoolNormFn take them at stages 2 and 3 of the encoder).

The pooled forms stage the same floats and zeros in the same LDS slots as the full-resolution entries do on
expand(dpool, amax), so every check here is bit for bit (torch.equal), never a tolerance:

* bwd-weight: each of the 14 non-wave-split rungs <TM, NBW> of conv_wgrad3_direct at the smallest shape
  tests/conv_models.py names for it, and the two anchors (32 -> 48 at 32 x 32; 48 -> 64 at 16 x 16, gx = 3) at Nb 1 and
  3, against sd_conv2d_wgrad_bf16x3 on the expanded tensor; the query names the same slab count.
* bwd-data: (48 -> 32, 32 x 32) and (64 -> 48, 16 x 16), Nb 1 and 3, against sd_conv2d_dgrad_direct on the expanded tensor.
* refusals: odd H, shapes outside the plans: the query says no, the entry returns SD_ESHAPE and launches nothing (the
  NaN-filled output stays NaN), and the stage takes the full-resolution route.
* stage level: both stage functions at the two anchor shapes, default route against ops.POOL_COMPACT off.

Inputs: dpool integer-valued (|v| <= 3), amax random in 0..3; with Nb >= 3 the last two images carry amax all 0 and all 3
(every border window at both parities of row and column). Outputs are NaN-filled before each launch."""
import pytest
import torch

import conv_models as cm

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (ci, co, H, W, k) -> the rung <tm, nbw> (and gx) direct3_plan gives it: the KERNEL_CASES that name a split-bf16 rung,
# and the two rungs only stage cases reach (co40: <3, 5>; film_fused's shape: <2, 4> at 8 x 8)
RUNG_SHAPES = {
    **{n: (c.ci, c.co, c.H, c.W, c.k) for n, c in cm.KERNEL.items()
       if c.op == "wgrad" and c.fast.startswith("conv_wgrad3_direct") and c.H % 2 == 0 and c.nb <= 3},
    "co40": tuple(getattr(cm.STAGE["co40"], f) for f in ("ci", "co", "H", "W", "k")),
    "film_fused": tuple(getattr(cm.STAGE["film_fused"], f) for f in ("ci", "co", "H", "W", "k")),
}
ANCHORS = {"a_32_48": (32, 48, 32, 32, 5), "a_48_64": (48, 64, 16, 16, 5)}
ALL_RUNGS = {(tm, nbw) for tm in (1, 2, 3, 4) for nbw in (2, 4, 5, 7) if tm <= 3 or nbw <= 4}


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _pooled_grad(nb, ho, wo, c, seed):
    """(dpool, amax, expand(dpool, amax)) on the device"""
    g = _g(seed)
    dpool = torch.randint(-3, 4, (nb, ho, wo, c), generator=g).float().to(DEV)
    amax = torch.randint(0, 4, (nb, ho, wo, c), generator=g, dtype=torch.uint8).to(DEV)
    if nb >= 3:
        amax[-2] = 0
        amax[-1] = 3
    full = torch.zeros(nb, 2 * ho, 2 * wo, c, device=DEV)
    for q in range(4):
        full[:, q >> 1::2, q & 1::2, :] = torch.where(amax == q, dpool, torch.zeros_like(dpool))
    return dpool, amax, full


def _wgrad_pair(ci, co, H, W, k, nb, seed):
    from sdreamer import _native as nat, kernels as K
    x = torch.randn(nb, H, W, ci, generator=_g(seed)).to(DEV)
    dpool, amax, full = _pooled_grad(nb, H // 2, W // 2, co, seed + 1)
    J, pad = k * k * ci, (k - 1) // 2
    ks = nat.fns["sd_conv2d_wgrad_bf16x3_slabs"](nb, H, W, ci, co, k, k, 0)
    assert ks > 0 and nat.fns["sd_conv2d_wgrad_bf16x3_pooled_slabs"](nb, H, W, ci, co, k, k) == ks
    outs = []
    for name, ptrs in (("sd_conv2d_wgrad_bf16x3", (K.p(x), K.p(full))),
                       ("sd_conv2d_wgrad_bf16x3_pooled", (K.p(x), K.p(dpool), K.p(amax)))):
        out = torch.full((co, J + 1), float("nan"), device=DEV)
        ws = torch.full((ks * co * (J + 1),), float("nan"), device=DEV)
        assert nat.call_shaped(name, *ptrs, K.p(out), K.p(ws), ws.numel(), nb, H, W, ci, co, k, k, pad, None, K.stream())
        outs.append(out)
    torch.cuda.synchronize()
    return outs


def test_the_rung_shapes_cover_every_non_ws_rung():
    got = set()
    for name, (ci, co, H, W, k) in RUNG_SHAPES.items():
        pl = cm.direct3_plan(3, H, W, ci, co, k, k)
        assert pl and not pl["ws"], name
        got.add((pl["tm"], pl["nbw"]))
    assert got == ALL_RUNGS and len(ALL_RUNGS) == 14, sorted(ALL_RUNGS - got)


@pytest.mark.parametrize("name", sorted(RUNG_SHAPES))
def test_pooled_wgrad_equals_full_resolution_at_every_rung(name):
    ci, co, H, W, k = RUNG_SHAPES[name]
    full, pooled = _wgrad_pair(ci, co, H, W, k, 3, seed=len(name))
    assert not torch.isnan(full).any() and torch.equal(pooled, full), name


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("name", sorted(ANCHORS))
def test_pooled_wgrad_equals_full_resolution_at_the_anchors(name, nb):
    ci, co, H, W, k = ANCHORS[name]
    pl = cm.direct3_plan(nb, H, W, ci, co, k, k)
    assert (pl["tm"], pl["nbw"], pl["gx"]) == ((3, 7, 1) if name == "a_32_48" else (4, 4, 3))
    full, pooled = _wgrad_pair(ci, co, H, W, k, nb, seed=7 + nb)
    assert not torch.isnan(full).any() and torch.equal(pooled, full), (name, nb)


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("cd,ci,hw", [(48, 32, 32), (64, 48, 16)])
def test_pooled_dgrad_equals_full_resolution(cd, ci, hw, nb):
    from sdreamer import _native as nat, kernels as K
    w = (torch.randn(cd, 5, 5, ci, generator=_g(cd + ci)) / (ci * 25) ** 0.5).to(DEV)
    ws = K.conv_split_weight(K.conv_flip_weight(w))
    dpool, amax, full = _pooled_grad(nb, hw // 2, hw // 2, cd, seed=hw + nb)
    assert nat.fns["sd_conv2d_dgrad_direct_pooled_ok"](hw, hw, cd, ci, 5, 5, 2) == 1
    ref = torch.full((nb, hw, hw, ci), float("nan"), device=DEV)
    got = torch.full((nb, hw, hw, ci), float("nan"), device=DEV)
    assert nat.call_shaped("sd_conv2d_dgrad_direct", K.p(full), K.p(ws), K.p(ref), nb, hw, hw, cd, ci, 5, 5, 2, K.stream())
    assert nat.call_shaped("sd_conv2d_dgrad_direct_pooled", K.p(dpool), K.p(amax), K.p(ws), K.p(got), nb, hw, hw, cd, ci,
                           5, 5, 2, K.stream())
    torch.cuda.synchronize()
    assert not torch.isnan(ref).any() and torch.equal(got, ref)
    assert torch.equal(K.conv2d_dgrad_pooled(dpool, amax, w), ref)  # the wrapper (its own flip + split of w)


@pytest.mark.parametrize("ci,co,H,W,k", [(16, 32, 3, 128, 3), (16, 32, 21, 16, 5), (4, 32, 16, 16, 5), (16, 96, 8, 8, 5),
                                         (16, 32, 12, 12, 5)])
def test_pooled_wgrad_refuses_outside_its_plan(ci, co, H, W, k):
    """odd H (3 x 128 is inside the full-resolution plan), H % R, Ci < 16, Co > 64, W no power of two"""
    from sdreamer import _native as nat, kernels as K
    nb, J = 2, k * k * ci
    assert nat.fns["sd_conv2d_wgrad_bf16x3_pooled_slabs"](nb, H, W, ci, co, k, k) == 0
    x = torch.randn(nb, H, W, ci, generator=_g(1)).to(DEV)
    dpool, amax, _ = _pooled_grad(nb, H // 2, W // 2, co, 2)
    out = torch.full((co, J + 1), float("nan"), device=DEV)
    ws = torch.full((4 * co * (J + 1),), float("nan"), device=DEV)
    rc = nat.fns["sd_conv2d_wgrad_bf16x3_pooled"](K.p(x), K.p(dpool), K.p(amax), K.p(out), K.p(ws), ws.numel(), nb, H, W,
                                                  ci, co, k, k, (k - 1) // 2, None, K.stream())
    torch.cuda.synchronize()
    assert rc == nat.SD_ESHAPE and torch.isnan(out).all() and torch.isnan(ws).all()
    with pytest.raises(nat.NativeError):
        K.conv2d_wgrad_pooled(x, dpool, amax, k, k)


@pytest.mark.parametrize("cd,ci,H,W,k", [(48, 32, 16, 16, 5), (64, 48, 32, 32, 5), (48, 32, 32, 32, 3), (32, 32, 32, 32, 5),
                                         (48, 32, 16, 32, 5)])
def test_pooled_dgrad_refuses_outside_its_shapes(cd, ci, H, W, k):
    from sdreamer import _native as nat, kernels as K
    nb = 2
    assert nat.fns["sd_conv2d_dgrad_direct_pooled_ok"](H, W, cd, ci, k, k, k - 1 - (k - 1) // 2) == 0
    w = torch.randn(cd, k, k, ci, generator=_g(3)).to(DEV)
    ws = K.conv_split_weight(K.conv_flip_weight(w))
    dpool, amax, _ = _pooled_grad(nb, H // 2, W // 2, cd, 4)
    din = torch.full((nb, H, W, ci), float("nan"), device=DEV)
    rc = nat.fns["sd_conv2d_dgrad_direct_pooled"](K.p(dpool), K.p(amax), K.p(ws), K.p(din), nb, H, W, cd, ci, k, k,
                                                  k - 1 - (k - 1) // 2, K.stream())
    torch.cuda.synchronize()
    assert rc == nat.SD_ESHAPE and torch.isnan(din).all()
    assert K.conv2d_dgrad_pooled(dpool, amax, w) is None


class _Spy:
    """counts the pooled wrappers' calls and records the element counts of the gradients the full-resolution bwd
    kernels' wrappers are given or return"""

    def __init__(self, monkeypatch):
        from sdreamer import kernels as K
        self.pooled, self.full = [], []
        for name in ("conv2d_wgrad_pooled", "conv2d_dgrad_pooled"):
            monkeypatch.setattr(K, name, self._wrap(getattr(K, name), name, self.pooled, None))
        monkeypatch.setattr(K, "conv2d_wgrad", self._wrap(K.conv2d_wgrad, "conv2d_wgrad", self.full, 1))
        monkeypatch.setattr(K, "conv2d_dgrad", self._wrap(K.conv2d_dgrad, "conv2d_dgrad", self.full, 0))
        monkeypatch.setattr(K, "pool_rms_bwd", self._wrap(K.pool_rms_bwd, "pool_rms_bwd", self.full, "out"))

    @staticmethod
    def _wrap(fn, name, log, which):
        def f(*a, **kw):
            out = fn(*a, **kw)
            t = None if which is None else (out[0] if isinstance(out, tuple) else out) if which == "out" else a[which]
            log.append((name, None if t is None else t.numel()))
            return out
        return f


def _run_stage(film, ci, co, hw, nb, dx, monkeypatch, compact):
    from sdreamer import ops
    monkeypatch.setattr(ops, "POOL_COMPACT", compact)
    spy = _Spy(monkeypatch)
    x = torch.randn(nb, hw, hw, ci, generator=_g(20)).to(DEV).requires_grad_(dx)
    w = (torch.randn(co, 5, 5, ci, generator=_g(21)) / (ci * 25) ** 0.5).to(DEV).requires_grad_()
    b = (0.1 * torch.randn(co, generator=_g(22))).to(DEV).requires_grad_()
    nw = (1 + 0.1 * torch.randn(co, generator=_g(23))).to(DEV).requires_grad_()
    leaves = [x, w, b, nw] if dx else [w, b, nw]
    if film:
        gamma = (1.5 + 0.2 * torch.randn(2, co, generator=_g(24))).to(DEV).requires_grad_()
        beta = (0.1 * torch.randn(2, co, generator=_g(25))).to(DEV).requires_grad_()
        leaves += [gamma, beta]
        y = ops.FilmConvPoolNormFn.apply(x, w, b, nw, gamma, beta, False)
    else:
        y = ops.ConvPoolNormFn.apply(x, w, b, nw, False)
    junk = [torch.full((nb, hw, hw, co), float("nan"), device=DEV) for _ in range(4)]  # what an unwritten dconv would hold
    torch.cuda.synchronize()
    del junk
    y.backward(torch.randn(y.shape, generator=_g(26)).to(DEV))
    torch.cuda.synchronize()
    monkeypatch.undo()
    return [t.grad.clone() for t in leaves], spy


@pytest.mark.parametrize("dx", [True, False])
@pytest.mark.parametrize("film", [False, True])
@pytest.mark.parametrize("name", sorted(ANCHORS))
def test_stage_pooled_route_equals_full_resolution_route(name, film, dx, monkeypatch):
    ci, co, hw, _, _ = ANCHORS[name]
    nb = 2
    got, spy = _run_stage(film, ci, co, hw, nb, dx, monkeypatch, True)
    ref, spy_off = _run_stage(film, ci, co, hw, nb, dx, monkeypatch, False)
    dconv = nb * hw * hw * co
    assert [n for n, _ in spy.pooled] == ["conv2d_wgrad_pooled"] + (["conv2d_dgrad_pooled"] if dx else [])
    assert not spy.full, spy.full  # no full-resolution conv gradient was formed or handed to a bwd kernel
    assert not spy_off.pooled and ("pool_rms_bwd", dconv) in spy_off.full and ("conv2d_wgrad", dconv) in spy_off.full
    what = (["dx"] if dx else []) + ["dw", "db", "dnw"] + (["dgamma", "dbeta"] if film else [])
    for n, a, r in zip(what, got, ref):
        assert not torch.isnan(r).any() and torch.equal(a, r), (name, n)


def test_stage_outside_the_pooled_plan_takes_the_full_resolution_route(monkeypatch):
    """21 x 16 (odd H: no pooled form of the bwd-weight) and a stage whose input gradient has no pooled form (16 -> 32 at
    16 x 16, dx wanted): the stage runs as before"""
    for ci, co, H, W, dx in ((16, 32, 21, 16, True), (16, 32, 16, 16, True)):
        from sdreamer import ops
        spy = _Spy(monkeypatch)
        x = torch.randn(2, H, W, ci, generator=_g(30)).to(DEV).requires_grad_(dx)
        w = (torch.randn(co, 5, 5, ci, generator=_g(31)) / 20).to(DEV).requires_grad_()
        b, nw = torch.zeros(co, device=DEV, requires_grad=True), torch.ones(co, device=DEV, requires_grad=True)
        y = ops.ConvPoolNormFn.apply(x, w, b, nw, False)
        y.backward(torch.randn(y.shape, generator=_g(32)).to(DEV))
        torch.cuda.synchronize()
        monkeypatch.undo()
        assert not spy.pooled and [n for n, _ in spy.full] == ["pool_rms_bwd", "conv2d_wgrad", "conv2d_dgrad"]
        assert not torch.isnan(x.grad).any() and not torch.isnan(w.grad).any()
