"""The imagination's serial backward on the GPU: ops._imag_walk_fused (the C entry sd_imagine_bwd, csrc/imgbwd.hip)
and ops._imag_walk_per_op on the same inputs against the float64 per-step reference (tests/imag_bwd_ref.py), for every
case that reaches the fused walk (imag_bwd_ref.FUSED_CASES):

    case            plan of the forward           what it adds
    dg64            k_hid<true> + k_lin6          Dg 64, N 65 (a one-row last tile), 3 actor / 2 img layers
    sk64_a16        k_hid<true> + k_lin6          N 1, SK 64, Kd 32, A 16 (32 actor logits), 1 actor / 4 img layers
    s68_onehot16    k_hid<false> + k_lin          one-hot actor A 16, S 68 (SK 1088)
    dg256_onehot1   k_hid_areg + k_lin6           one-hot actor A 1, 4 actor / 1 img layers, Kd 32
    areg_h2         k_hid_areg + k_lin6_areg      the workload's plan (D 2048, G 8), one step
    anchor_n33_h4   k_hid_areg + k_lin6_areg      the workload's plan, N 33, three steps
per_op_dg96 / per_op_dg32 are outside the gate and take the per-op walk.

Per step and tensor the bound is GRAD_REL * max|ref| + GRAD_ABS; both upstreams; the product's imagined indices equal
the reference's exactly. Largest fraction of the bound measured on an MI355X (printed per case by
test_walks_match_float64_reference): the fused walk 0.0060 (areg_h2; the others 0.0004 .. 0.0019), the per-op walk on
the same inputs 0.0058 (areg_h2; the others 0.0002 .. 0.0018); DESIGN.md § 4.4c records both."""

import numpy as np
import pytest
import torch

import imag_bwd_ref as ibr
import small_models as sm
from launch_trace import recorded

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = [c.name for c in ibr.FUSED_CASES]
_SETUP = {}


def setup(c):
    """the product, its forward rollout and the batched recompute of case c (computed once, left unchanged)"""
    if c not in _SETUP:
        from sdreamer import ops
        ag = sm.build_product(c)
        stoch, deter = sm.imag_inputs(c)
        with torch.no_grad():
            feats, actions = ag._imagine_tm((stoch.to(DEV).reshape(c.N, -1), deter.to(DEV)), c.H1, sm.noise_seed(c),
                                            sm.IMAG_ROW_OFFSET)
            rec = ops._imag_recompute(ag, feats, actions, c.H1)
        torch.cuda.synchronize()
        _SETUP[c] = (ag, feats, actions, rec)
    return _SETUP[c]


def grads_in(c, which):
    g = ibr.upstream(c, which).float().to(DEV)
    SK = c.S * c.K
    return g[..., :SK].contiguous(), g[..., SK:].contiguous()


def walk(c, which, fused, **kw):
    from sdreamer import ops
    ag, _, _, rec = setup(c)
    d_st, d_de = grads_in(c, which)
    fn = ops._imag_walk_fused if fused else ops._imag_walk_per_op
    fn(ag, rec, d_st, d_de, sm.noise_seed(c), sm.IMAG_ROW_OFFSET, **kw)
    torch.cuda.synchronize()
    return d_st, d_de


def _fraction(c, which, fused):
    ref = ibr.cached(c, torch.float64, which)
    d_st, d_de = walk(c, which, fused)
    return ibr.step_fractions(d_st.cpu().numpy().astype(np.float64), d_de.cpu().numpy().astype(np.float64), ref)


@pytest.mark.parametrize("c", ibr.FUSED_CASES, ids=IDS)
def test_walks_match_float64_reference(c):
    from sdreamer import ops
    ag, feats, actions, rec = setup(c)
    assert ag._fused_imag_ok() and ops.imag_walk_is_fused(ag, rec)
    ref = ibr.cached(c, torch.float64, "last")
    SK = c.S * c.K
    idx = feats[..., :SK].reshape(c.H1, c.N, c.S, c.K).argmax(-1).cpu().numpy()
    assert np.array_equal(idx, ref["idx"]), "imagined indices differ"
    if c.discrete:
        assert np.array_equal(actions.argmax(-1).cpu().numpy(), ref["actions"].argmax(-1)), "one-hot actions differ"
    worst = {}
    for fused in (True, False):
        fr = np.stack([_fraction(c, which, fused) for which in ibr.UPSTREAMS])
        worst[fused] = fr.max()
        print(f"{c.name}: {'fused' if fused else 'per-op'} walk uses at most {fr.max():.4f} of the bound "
              f"(per step, last / all: {np.round(fr, 4).tolist()})", flush=True)
    # the per-op walk first: a failure of the reference shows there too, a failure of the fused walk only below
    assert worst[False] <= 1.0, (c.name, "per-op walk", worst[False])
    assert worst[True] <= 1.0, (c.name, "fused walk", worst[True])


@pytest.mark.parametrize("c", ibr.FUSED_CASES, ids=IDS)
def test_two_fused_calls_give_the_same_bits(c):
    a, b = walk(c, "all", True), walk(c, "all", True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("c", [c for c in ibr.FUSED_CASES if c.H1 > 2], ids=lambda c: c.name)
def test_chunked_call_gives_the_unchunked_bits(c):
    whole = walk(c, "all", True)
    for k in range(1, c.H1 - 1):
        parts = walk(c, "all", True, chunks=[0, k, c.H1 - 1])
        assert torch.equal(whole[0], parts[0]) and torch.equal(whole[1], parts[1]), k


def test_graph_replay_gives_the_eager_bits():
    from sdreamer import ops
    c = sm.IMAG["dg64"]
    ag, _, _, rec = setup(c)
    g_st, g_de = grads_in(c, "all")
    d_st, d_de = g_st.clone(), g_de.clone()
    args = (ag, rec, d_st, d_de, sm.noise_seed(c), sm.IMAG_ROW_OFFSET)
    work = ops._imag_walk_fused(*args)
    torch.cuda.synchronize()
    eager = d_st.clone(), d_de.clone()
    d_st.copy_(g_st)
    d_de.copy_(g_de)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream: the entry allocates nothing and never synchronises
        ops._imag_walk_fused(*args, work=work)
    d_st.copy_(g_st)
    d_de.copy_(g_de)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(d_st, eager[0]) and torch.equal(d_de, eager[1])


def test_shape_outside_the_gate_is_refused_before_any_launch():
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    from sdreamer import ops
    c = ibr.OUTSIDE
    ag, _, _, rec = setup(c)
    assert not ag._fused_imag_ok() and not ops.imag_walk_is_fused(ag, rec)
    SK = c.S * c.K
    d_st = torch.full((c.H1, c.N, SK), 7.0, device=DEV)
    d_de = torch.full((c.H1, c.N, c.D), 7.0, device=DEV)
    work = torch.full((1 << 16,), 7.0, device=DEV)
    d, _hold, addr = ops._imag_bwd_desc(ag, rec, d_st, d_de, sm.noise_seed(c), sm.IMAG_ROW_OFFSET)
    d.work = work.data_ptr()
    assert nat.fns["sd_imagine_bwd_ok"](addr) == 0
    assert nat.fns["sd_imagine_bwd_work_floats"](addr) == nat.SD_ESHAPE < 0
    assert nat.fns["sd_imagine_bwd"](addr, K.stream()) == nat.SD_ESHAPE
    torch.cuda.synchronize()
    for t in (d_st, d_de, work):
        assert bool((t == 7.0).all())


def _backward_launches(c):
    ag = setup(c)[0]
    stoch, deter = sm.imag_inputs(c)
    s, d = stoch.to(DEV).requires_grad_(True), deter.to(DEV).requires_grad_(True)
    ret0 = ag.imagined_return(s, d, horizon=c.H1 - 1, seed=sm.noise_seed(c), row_offset=sm.IMAG_ROW_OFFSET)
    _, names = recorded(lambda: ret0.sum().backward())
    assert bool(torch.isfinite(s.grad).all()) and bool(torch.isfinite(d.grad).all())
    return names


def test_route():
    per_op = ("sd_gru_bwd", "sd_onehot_sample_bwd", "sd_bnormal_sample_bwd")
    names = _backward_launches(sm.IMAG["dg64"])
    assert names.count("sd_imagine_bwd") == 1 and not any(n in names for n in per_op), names
    names = _backward_launches(ibr.OUTSIDE)
    assert "sd_gru_bwd" in names and "sd_imagine_bwd" not in names, names
