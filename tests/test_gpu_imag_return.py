"""Dreamer.imagined_return (ops.ImagineReturnFn) on the small imagination cases against the float64 oracle under
autograd (tests/imag_return_ref.py), the forward against the no-grad path bit for bit, and the update left alone.

What the cases reach (small_models.IMAG_CASES): both actor kinds (bounded normal: dg64, sk64_a16, areg_h2, the per-op
pair; one-hot: s68_onehot16, dg256_onehot1), A = 1 (dg256_onehot1, areg_h2), N = 1 (sk64_a16), H1 = 2 (areg_h2),
S > 64 (s68_onehot16) and the two shapes outside the fused imagination's gate (per_op_dg96, per_op_dg32).

Fractions of the gradient bound GRAD_REL * max|ref| + GRAD_ABS used on an MI355X (printed per case by
test_matches_float64_oracle): at most 0.0054 (areg_h2 d_stoch; the others 0.0003 .. 0.0042) with the heads' batched
contractions on split-bf16, 0.0045 with every contraction on exact f32; ret0 at most 0.0008 of its bound. The float32
oracle itself uses 0.0006 (tests/test_imag_return_cpu.py). DESIGN.md §4.4c records the largest."""
import numpy as np
import pytest
import torch

import small_models as sm
from launch_trace import recorded as _recorded
from test_imag_return_cpu import cached, upstream

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _product(c, ag=None):
    ag = ag or sm.build_product(c)
    stoch, deter = sm.imag_inputs(c)
    s, d = stoch.to(DEV).requires_grad_(True), deter.to(DEV).requires_grad_(True)
    keep = {}
    ret0 = ag.imagined_return(s, d, horizon=c.H1 - 1, seed=sm.noise_seed(c), row_offset=sm.IMAG_ROW_OFFSET, keep=keep)
    u = torch.from_numpy(upstream(c)).float().to(DEV)
    gs, gd = torch.autograd.grad((ret0 * u).sum(), [s, d])
    torch.cuda.synchronize()
    return ag, ret0.detach(), gs, gd, keep


@pytest.mark.parametrize("c", sm.IMAG_CASES, ids=lambda c: c.name)
def test_matches_float64_oracle(c):
    ref = cached(c, torch.float64)
    ag, ret0, gs, gd, keep = _product(c)
    assert bool(ag._fused_imag_ok()) == c.fused
    SK = c.S * c.K
    f, a = keep["feats"], keep["actions"]
    assert f.shape == (c.H1, c.N, SK + c.D) and a.shape == (c.H1, c.N, c.A) and ret0.shape == (c.N,)
    idx = f[..., :SK].reshape(c.H1, c.N, c.S, c.K).argmax(-1).cpu().numpy()
    assert np.array_equal(idx, ref["idx"]), "imagined indices differ"
    if c.discrete:
        assert np.array_equal(a.argmax(-1).cpu().numpy(), ref["actions"].argmax(-1)), "one-hot actions differ"
    r = sm._ratio(ret0.cpu().numpy().astype(np.float64), ref["ret0"], sm.IMAG_RTOL, sm.IMAG_ATOL)
    assert r <= 1.0, f"ret0 uses {r:.3g} of the {sm.IMAG_ATOL} + {sm.IMAG_RTOL} |ref| bound"
    fr = {}
    for k, g in (("d_stoch", gs), ("d_deter", gd)):
        assert g.shape == ref[k].shape
        e, s = sm._rel_max(g.cpu().numpy().astype(np.float64), ref[k])
        fr[k] = e / (sm.GRAD_REL * s + sm.GRAD_ABS)
    print(f"{c.name}: ret0 {r:.4f} of its bound; d_stoch {fr['d_stoch']:.4f}, d_deter {fr['d_deter']:.4f} of the "
          f"gradient bound", flush=True)
    assert max(fr.values()) <= 1.0, (c.name, fr)


def test_forward_is_the_no_grad_path_bit_for_bit():
    c = sm.IMAG["dg64"]
    ag, ret0, _, _, keep = _product(c)
    assert ag._fused_imag_ok()
    stoch, deter = sm.imag_inputs(c)
    with torch.no_grad():
        f, a = ag._imagine_tm((stoch.to(DEV), deter.to(DEV)), c.H1, sm.noise_seed(c), sm.IMAG_ROW_OFFSET)
        rr = ag._heads_returns(f)
    torch.cuda.synchronize()
    assert torch.equal(f, keep["feats"]) and torch.equal(a, keep["actions"]) and torch.equal(rr["ret"], keep["ret"])
    assert torch.equal(ret0, rr["ret"][:, 0])
    # and the same bits on repetition, gradients included
    _, ret0b, gs, gd, _ = _product(c, ag)
    _, ret0c, gs2, gd2, _ = _product(c, ag)
    assert torch.equal(ret0b, ret0) and torch.equal(ret0c, ret0) and torch.equal(gs, gs2) and torch.equal(gd, gd2)


@pytest.mark.parametrize("sink", [False, True], ids=["bare", "grad_sink_scope"])
def test_update_is_untouched(sink):
    """An eager update, a backward of imagined_return, another eager update: the gradient arena, every param.grad
    and _grads_clean are as the first update left them after the backward, and the second update issues the
    launches of the first, in the same order."""
    import contextlib
    from golden_io import batch, initial
    from sdreamer import ops
    from test_gpu_dreamer import build_agent
    ag, z, spec, obs = build_agent("walker_r2")
    ag.use_graphs = False
    data, init = batch(z, 0, obs, DEV), initial(z, 0, spec, DEV)
    ag.update_batch(data, init, 11)  # warm-up: one-time work (buffers, cached layouts) is done
    _, first = _recorded(lambda: ag.update_batch(data, init, 12))
    arena = ag._optimizer.arena.grad.clone()
    grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in ag.named_parameters()}
    clean = ag._grads_clean
    ps, pd, _ = ag.posterior(data, init, seed=5)
    s, d = ps.detach().clone().requires_grad_(True), pd.detach().clone().requires_grad_(True)
    with (ops.grad_sink_scope() if sink else contextlib.nullcontext()):
        (ret0, names) = _recorded(lambda: ag.imagined_return(s, d, seed=5))
        _, bwd = _recorded(lambda: ret0.mean().backward())
    assert ret0.shape == (ps.shape[0] * ps.shape[1],)
    assert bool(torch.isfinite(s.grad).all()) and bool(d.grad.abs().sum() > 0) and bool(s.grad.abs().sum() > 0)
    assert "sd_lambda_return_bwd" in bwd and "sd_twohot_mode_bwd" in bwd and "sd_lambda_return_strided" in names
    assert "sd_imagine_run" not in bwd and "sd_onehot_sample_fwd" not in bwd and "sd_bnormal_sample" not in bwd
    assert ops._GRAD_SINK is None
    assert torch.equal(ag._optimizer.arena.grad, arena) and ag._grads_clean == clean
    for k, p in ag.named_parameters():
        assert (p.grad is None) == (grads[k] is None), k
        assert p.grad is None or torch.equal(p.grad, grads[k]), k
    _, second = _recorded(lambda: ag.update_batch(data, init, 13))
    assert len(first) > 100 and first == second
    assert not any(n in first for n in ("sd_lambda_return_bwd", "sd_twohot_mode_bwd", "sd_bnormal_sample_bwd"))
