"""The per-step reference of the imagination's serial backward (tests/imag_bwd_ref.py) on the CPU, for every case that
reaches the fused walk (imag_bwd_ref.FUSED_CASES: the fused small_models.IMAG_CASES and anchor_n33_h4):

 1. the float32 oracle against the float64 oracle uses at most ROOM = 0.25 of the GPU bound
    (GRAD_REL * max|ref| + GRAD_ABS per step and tensor) at every step, with both upstreams;
 2. the mutations no_straight_through and eps_zero (continuous actors only) exceed that bound at every step t < H
    (d_deter[t], and d_stoch[t] where the mutated rollout still defines it: a detached sample has no gradient);
 3. anchor_n33_h4's seed is the first of 0, 1, 2, ... that meets small_models' input condition."""
import numpy as np
import pytest
import torch

import imag_bwd_ref as ibr
import small_models as sm

ROOM = 0.25
IDS = [c.name for c in ibr.FUSED_CASES]


def test_cases_reach_the_gate():
    names = set(IDS)
    assert {"areg_h2", "dg64", "anchor_n33_h4"} <= names and any(c.discrete for c in ibr.FUSED_CASES)
    for c in ibr.FUSED_CASES:
        assert sm.imag_plan(c) == c.plan != "per-op", c.name
    assert sm.imag_plan(ibr.OUTSIDE) == "per-op"
    a = ibr.ANCHOR
    assert (a.D, a.G, a.S, a.K, a.A, a.discrete, a.actor_layers, a.img_layers, a.N, a.H1) == \
        (2048, 8, 32, 16, 6, False, 3, 2, 33, 4)


def _condition(c):
    """small_models' input rule on the float32 / float64 rollouts of case c -> (margin, same indices)"""
    r32, r64 = ibr.cached(c, torch.float32, "last"), ibr.cached(c, torch.float64, "last")
    same = np.array_equal(r32["idx"], r64["idx"])
    if c.discrete:
        same = same and np.array_equal(r32["actions"].argmax(-1), r64["actions"].argmax(-1))
    return sm.imag_min_margin(c, r32), same


def test_anchor_seed_is_the_first_that_meets_the_input_condition():
    import dataclasses
    for seed in range(ibr.ANCHOR.seed):
        m, same = _condition(dataclasses.replace(ibr.ANCHOR, seed=seed))
        assert m < sm.MIN_MARGIN or not same, f"seed {seed} already meets the condition (margin {m:.3g})"
    m, same = _condition(ibr.ANCHOR)
    assert m >= sm.MIN_MARGIN and same, (m, same)


@pytest.mark.parametrize("c", ibr.FUSED_CASES, ids=IDS)
def test_float32_oracle_leaves_room_at_every_step(c):
    worst = 0.0
    for which in ibr.UPSTREAMS:
        r32, r64 = ibr.cached(c, torch.float32, which), ibr.cached(c, torch.float64, which)
        assert np.array_equal(r32["idx"], r64["idx"])
        tops = [max(np.abs(r64["d_stoch"][t]).max(), np.abs(r64["d_deter"][t]).max()) for t in range(c.H1)]
        assert min(tops) > 0, tops  # the bound is not vacuous: every step's total is nonzero
        fr = ibr.step_fractions(r32["d_stoch"], r32["d_deter"], r64)
        print(f"{c.name} [{which}]: float32 oracle uses at most {fr.max():.4f} of the bound; per-step maxima "
              f"{min(tops):.3g} .. {max(tops):.3g}", flush=True)
        worst = max(worst, fr.max())
    assert worst <= ROOM, (c.name, worst)


@pytest.mark.parametrize("c", ibr.FUSED_CASES, ids=IDS)
def test_bound_catches_mutations_at_every_step(c):
    for which in ibr.UPSTREAMS:
        r64 = ibr.cached(c, torch.float64, which)
        for m in ibr.applicable(c):
            mut = ibr.run(c, torch.float64, which, m)
            fr = ibr.step_fractions(mut["d_stoch"], mut["d_deter"], r64, mut["has_stoch"])[:c.H1 - 1]
            print(f"{c.name} [{which}]: mutation {m} is {fr.min():.3g} .. {fr.max():.3g} of the bound over t < H",
                  flush=True)
            assert fr.min() > 1.0, (c.name, which, m, fr)
