"""Per-step reference of the imagination's serial backward (ops._imag_walk_fused / _imag_walk_per_op, the C entry
sd_imagine_bwd): tests/imag_return_ref.rollout on the CPU oracle under autograd, with every step's (stoch_t, deter_t)
recorded as the rollout reads them. Test infrastructure, not a test.

With an upstream g (H1, N, F) the objective is sum_t <feat_t, g_t>; the reference for step t is autograd.grad of it
with respect to the STATE tensors (stoch_t, deter_t), not the feat tensor: deter_step consumes stoch and deter
directly, and a gradient taken at feat would miss the whole recurrent path. That is the walk's contract: on entry
d_stoch[t] / d_deter[t] hold g_t, on exit the total gradient at step t's state.

Two upstreams (seeded randn): "last" (g_t = 0 for t < H: every earlier step's total is purely propagated) and "all"
(g_0 = 0, the rest random: the accumulate-in-place contract)."""
import numpy as np
import torch

import imag_return_ref as irr
import small_models as sm
from oracle.ref_cpu import Oracle

PREFIXES = ("rssm.", "actor.")
UPSTREAMS = ("last", "all")
MUTATIONS = ("no_straight_through", "eps_zero")

# the workload's plan (D 2048, G 8, 32 x 16 latents, bounded-normal A 6) on 33 rows (a partial last row tile behind
# full ones) and three serial steps, so the carried gradient crosses more than one step on that plan.
# seed: the first of 0, 1, 2, ... that meets small_models' input condition (test_imag_bwd_cpu.py asserts it)
ANCHOR = sm.ImagCase("anchor_n33_h4", 2048, 8, 32, 16, 6, False, 3, 2, 33, 4, True, "k_hid_areg + k_lin6_areg", seed=0)
# which cases reach the fused walk: every IMAG_CASES entry inside the fused imagination's gate (sd_imagine_bwd_ok
# admits exactly sd_imagine's shapes with H1 >= 2), and the anchor
FUSED_CASES = [c for c in sm.IMAG_CASES if c.fused] + [ANCHOR]
OUTSIDE = sm.IMAG["per_op_dg96"]


def upstream(c, which):
    """g (H1, N, SK + D) float64"""
    assert which in UPSTREAMS
    g = torch.randn(c.H1, c.N, c.S * c.K + c.D, generator=torch.Generator().manual_seed(977 + c.seed)).double()
    if which == "last":
        g[:c.H1 - 1] = 0
    else:
        g[0] = 0
    return g


def applicable(c):
    return [m for m in MUTATIONS if m != "eps_zero" or not c.discrete]


def run(c, dtype, which, mutate=None):
    """-> dict: d_stoch (H1, N, SK), d_deter (H1, N, D) float64 (the per-step totals), has_stoch (H1,) bool (a mutated
    rollout detaches its samples: no gradient is defined at those state tensors), idx (H1, N, S), actions (H1, N, A)
    and the logits the margins need"""
    stoch, deter = sm.imag_inputs(c)
    SK = c.S * c.K
    with sm.oracle_dtype(dtype):
        orc, _ = sm._oracle(c, dtype, Oracle, PREFIXES)
        states, inner = [], orc.get_feat

        def get_feat(s, d):
            states.append((s, d))
            return inner(s, d)

        orc.get_feat = get_feat
        s0 = stoch.to(dtype).clone().requires_grad_(True)
        d0 = deter.to(dtype).clone().requires_grad_(True)
        feats, actions, plogits, alogits = irr.rollout(orc, (s0, d0), c.H1, sm.noise_seed(c), sm.IMAG_ROW_OFFSET,
                                                       mutate)
        assert len(states) == c.H1
        g = upstream(c, which).to(dtype)
        obj = (feats * g.transpose(0, 1)).sum()
        wanted = [x for sd in states for x in sd if x.requires_grad]
        grads = iter(torch.autograd.grad(obj, wanted, allow_unused=True))
    f64 = lambda t: t.detach().numpy().astype(np.float64)  # noqa: E731
    d_st, d_de, has = np.zeros((c.H1, c.N, SK)), np.zeros((c.H1, c.N, c.D)), np.zeros(c.H1, bool)
    for t, (s, d) in enumerate(states):
        if s.requires_grad:
            gs = next(grads)
            d_st[t], has[t] = (0 if gs is None else f64(gs).reshape(c.N, SK)), True
        gd = next(grads)
        d_de[t] = 0 if gd is None else f64(gd)
    ft = feats.detach().transpose(0, 1)
    return dict(d_stoch=d_st, d_deter=d_de, has_stoch=has,
                idx=ft[..., :SK].reshape(c.H1, c.N, c.S, c.K).argmax(-1).numpy(),
                actions=f64(actions.transpose(0, 1)), actor_logit=f64(torch.stack(alogits, 1)),
                prior_logit=f64(torch.stack(plogits, 1)))


_CACHE = {}


def cached(c, dtype, which):
    """the unmutated reference, computed once and shared (callers leave it unchanged)"""
    if (c, dtype, which) not in _CACHE:
        _CACHE[c, dtype, which] = run(c, dtype, which)
    return _CACHE[c, dtype, which]


def step_fractions(got_st, got_de, ref, has_stoch=None):
    """(H1,) array: per step, the larger fraction of GRAD_REL * max|ref| + GRAD_ABS used by d_stoch[t] / d_deter[t]
    (got_*: float64 arrays shaped like the reference's; has_stoch: steps whose d_stoch is judged, default all)"""
    H1 = ref["d_deter"].shape[0]
    out = np.zeros(H1)
    for t in range(H1):
        pairs = [(got_de[t], ref["d_deter"][t])]
        if has_stoch is None or has_stoch[t]:
            pairs.append((got_st[t], ref["d_stoch"][t]))
        for got, want in pairs:
            e, s = sm._rel_max(got, want)
            out[t] = max(out[t], e / (sm.GRAD_REL * s + sm.GRAD_ABS))
    return out
