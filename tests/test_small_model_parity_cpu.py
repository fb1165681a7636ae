"""CPU self-check of the small-model parity tests (tests/small_models.py; test_gpu_scan_f64.py and
test_gpu_imagine_f64.py run the same cases and comparisons on the product). For every case:

1. the input condition that lets the GPU tests demand exact index equality with no row excluded: under the float32
   oracle every categorical's top-2 perturbed-logit margin is >= 1e-4 (ten times parity.MARGIN), and the float32 and
   float64 oracles draw the same indices. A case that fails this gets another seed in small_models.py;
2. the comparison functions pass the float32 oracle against the float64 one (it sits about three orders of magnitude
   inside the caps);
3. they fail on deliberately wrong float32 oracles: a reset ignored for one row at one step, the last block's
   recurrent input taken from the block before it, the initial state replaced by zeros (scan and imagination), and
   for the imagination, which has no resets, the noise counters' row offset dropped. Where a mutation cannot change
   a case (one row and one step cannot both read the initial state and be reset: the two t1_b1 cases split that; the
   reset one has no recurrent input at all), the test asserts that the mutant equals the float32 oracle there, so the exception is checked, not skipped.

The C side of the imagination's shape gate (sd_imagine_work_floats, which launches nothing) is checked here too.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_models as sm
from oracle.ref_cpu import Oracle, block_linear, rms

F32, F64 = torch.float32, torch.float64
SCAN_IDS = [c.name for c in sm.SCAN_CASES]
IMAG_IDS = [c.name for c in sm.IMAG_CASES]


# --------------------------------------------------------------------------------------------------- mutated oracles
class ResetIgnored(Oracle):
    """the reset flag of (row, step) is not applied: that row's state and action go through as they are"""
    at = (0, 0)

    def observe(self, embed, action, initial, reset, *a, **k):
        reset = reset.clone()
        reset[self.at] = False
        return super().observe(embed, action, initial, reset, *a, **k)


class ZeroInitial(Oracle):
    """the initial (scan) / start (imagination) state is replaced by zeros"""

    def observe(self, embed, action, initial, *a, **k):
        return super().observe(embed, action, tuple(torch.zeros_like(x) for x in initial), *a, **k)

    def imagine(self, start, *a, **k):
        return super().imagine(tuple(torch.zeros_like(x) for x in start), *a, **k)


class WrongBlock(Oracle):
    """Deter.forward with the last block's recurrent input (the block-diagonal operand of dyn_hid only) taken from the
    block before it: what a column tile that straddles two blocks computes. With one block, the block's second half
    of columns takes the first half's."""

    def deter_step(self, stoch, deter, action, P=None):
        s = self.s
        P = P or self.P
        pre = "rssm._deter_net."
        B = action.shape[0]
        stoch = stoch.reshape(B, -1)
        action = action / torch.clip(torch.abs(action), min=1.0).detach()

        def inp(nm, x):
            return F.silu(rms(F.linear(x, P[pre + nm + ".0.weight"], P[pre + nm + ".0.bias"]), P[pre + nm + ".1.weight"]))

        x0, x1, x2 = inp("_dyn_in0", deter), inp("_dyn_in1", stoch), inp("_dyn_in2", action)
        x = torch.cat([x0, x1, x2], -1).unsqueeze(-2).expand(-1, s.G, -1)
        unit = s.D // s.G if s.G > 1 else s.D // 2
        hb = torch.cat([deter[:, :s.D - unit], deter[:, s.D - 2 * unit:s.D - unit]], -1)  # the mutation
        x = torch.cat([hb.reshape(B, s.G, -1), x], -1).reshape(B, -1)
        x = block_linear(x, P[pre + "_dyn_hid.dyn_hid_0.weight"], P[pre + "_dyn_hid.dyn_hid_0.bias"], s.G)
        x = F.silu(rms(x, P[pre + "_dyn_hid.norm_0.weight"]))
        x = block_linear(x, P[pre + "_dyn_gru.weight"], P[pre + "_dyn_gru.bias"], s.G)
        reset, cand, update = (g.reshape(B, -1) for g in torch.chunk(x.reshape(B, s.G, -1), 3, dim=-1))
        cand = torch.tanh(torch.sigmoid(reset) * cand)
        update = torch.sigmoid(update - 1)
        return update * cand + (1 - update) * deter


class RowOffsetDropped(Oracle):
    """the imagined rows' noise counters start at global row 0, not at the call's row offset"""

    def imagine(self, start, horizon, seed, row_offset=0, rec=None):
        return super().imagine(start, horizon, seed, 0, rec)


def test_wrong_block_restates_deter_step_but_for_the_mutation():
    """the mutant's copy of Deter.forward is the oracle's when the mutated operand is put back"""
    c = sm.SCAN["kd64_sk512"]
    spec, params = sm.spec_params(c)
    P = {k: torch.tensor(v) for k, v in params.items() if k.startswith("rssm.")}
    g = torch.Generator().manual_seed(1)
    deter = torch.randn(3, c.D, generator=g)
    deter[:, c.D - c.Dg:] = deter[:, c.D - 2 * c.Dg:c.D - c.Dg]  # the last block already equals the one before it
    stoch, act = torch.randn(3, c.S * c.K, generator=g), torch.randn(3, c.A, generator=g)
    assert torch.equal(WrongBlock(spec, P).deter_step(stoch, deter, act), Oracle(spec, P).deter_step(stoch, deter, act))


# --------------------------------------------------------------------------------------------------- the cases
def test_case_tables():
    """the shapes the issue lists, the gates' expectation per case, and the reset / initial-state edges"""
    for c in sm.SCAN_CASES:
        fused = c.Dg in (256, 512) and c.S * c.K in (512, 1024) and c.K in (16, 32, 64) and c.D % c.K == 0
        assert fused == c.fused, c.name
        reset = sm.scan_inputs(c)[2]
        if c.B >= 3:  # a row never reset (reads the initial state), one reset at every step, one at step T - 1 only
            rows = [tuple(r.tolist()) for r in reset]
            assert (False,) * c.T in rows and (True,) * c.T in rows and (False,) * (c.T - 1) + (True,) in rows, c.name
    assert not sm.scan_inputs(sm.SCAN["t1_b1_init"])[2].any() and sm.scan_inputs(sm.SCAN["t1_b1_reset"])[2].all()
    for c in sm.IMAG_CASES:
        assert sm.imag_plan(c) == c.plan and (c.plan != "per-op") == c.fused, c.name
    assert {c.plan for c in sm.IMAG_CASES} == {"k_hid<true> + k_lin6", "k_hid<false> + k_lin", "k_hid_areg + k_lin6",
                                               "k_hid_areg + k_lin6_areg", "per-op"}


@pytest.mark.parametrize("name", SCAN_IDS)
def test_scan_inputs_have_no_near_ties(name):
    c = sm.SCAN[name]
    r32, r64 = sm.run_oracle_scan(c, F32), sm.run_oracle_scan(c, F64)
    m = sm.scan_min_margin(c, r32)
    print(f"{name}: smallest posterior margin {m:.3g}")
    assert m >= sm.MIN_MARGIN, f"{name}: margin {m:.3g} < {sm.MIN_MARGIN}: choose another seed"
    assert np.array_equal(r32["idx"], r64["idx"])


@pytest.mark.parametrize("name", SCAN_IDS)
def test_scan_float32_oracle_passes(name):
    c = sm.SCAN[name]
    err = sm.compare_scan(sm.run_oracle_scan(c, F32), sm.run_oracle_scan(c, F64), name)
    print(name, sm.scan_summary(err))
    s = sm.scan_summary(err)
    assert s["state_abs"] < 1e-5 and s["embed_rel"] < 1e-5 and s["param_rel"] < 1e-5  # far inside the caps


@pytest.mark.parametrize("combo", sm.GRAD_COMBOS, ids=["+".join(g) for g in sm.GRAD_COMBOS])
def test_scan_partial_grads_float32_oracle_passes(combo):
    c = sm.SCAN["kd64_sk512"]
    full = sm.run_oracle_scan(c, F64)
    part = sm.run_oracle_scan(c, F64, combo)
    sm.compare_scan(sm.run_oracle_scan(c, F32, combo), part, f"{c.name} {combo}")
    with pytest.raises(AssertionError):  # and the partial loss is another function: its gradient is not the full one
        sm.compare_scan(full, part)


def _reset_site(c):
    """(row, step) of a reset that matters: the row reset at every step, at the last step (its state then is the
    previous step's posterior, or the initial state when T = 1); None if the case has no such row"""
    reset = sm.scan_inputs(c)[2]
    rows = [r for r in range(c.B) if bool(reset[r].all())]
    return (rows[0], c.T - 1) if rows else None


def _scan_mutants(c):
    """name -> (class, attributes, whether the mutation can change this case's outputs)"""
    reset = sm.scan_inputs(c)[2]
    site = _reset_site(c)
    return {"reset_ignored": (ResetIgnored, dict(at=site or (0, 0)), site is not None),
            # (a recurrent input exists: some row's state is not zeroed before the only step)
            "wrong_block": (WrongBlock, {}, c.T > 1 or bool((~reset[:, 0]).any())),
            "zero_initial": (ZeroInitial, {}, bool((~reset[:, 0]).any()))}


def test_mutations_apply_to_every_scan_case_but_the_single_step_pair():
    for c in sm.SCAN_CASES:
        off = sorted(k for k, (_, _, applies) in _scan_mutants(c).items() if not applies)
        assert off == {"t1_b1_init": ["reset_ignored"], "t1_b1_reset": ["wrong_block", "zero_initial"]}.get(c.name, []), c.name


@pytest.mark.parametrize("mut", ["reset_ignored", "wrong_block", "zero_initial"])
@pytest.mark.parametrize("name", SCAN_IDS)
def test_scan_comparison_fails_on_wrong_oracle(name, mut):
    c = sm.SCAN[name]
    cls, attrs, applies = _scan_mutants(c)[mut]
    wrong = sm.run_oracle_scan(c, F32, cls=cls, **attrs)
    if not applies:  # nothing for the mutation to change here: it must then BE the float32 oracle
        r32 = sm.run_oracle_scan(c, F32)
        assert np.array_equal(wrong["deter"], r32["deter"]) and np.array_equal(wrong["d_embed"], r32["d_embed"])
        return
    with pytest.raises(AssertionError):
        sm.compare_scan(wrong, sm.run_oracle_scan(c, F64), f"{name} {mut}")
    # and not through the sampled indices alone: the states or the gradients miss their caps too
    err = sm.scan_errors(wrong, sm.run_oracle_scan(c, F64))
    s = sm.scan_summary(err)
    assert err["state_ratio"] > 1 or s["embed_rel"] > sm.GRAD_REL or s["param_rel"] > sm.GRAD_REL, s


@pytest.mark.parametrize("name", IMAG_IDS)
def test_imag_inputs_have_no_near_ties(name):
    c = sm.IMAG[name]
    r32, r64 = sm.run_oracle_imag(c, F32), sm.run_oracle_imag(c, F64)
    m = sm.imag_min_margin(c, r32)
    print(f"{name}: smallest prior / action margin {m:.3g}")
    assert m >= sm.MIN_MARGIN, f"{name}: margin {m:.3g} < {sm.MIN_MARGIN}: choose another seed"
    assert np.array_equal(r32["idx"], r64["idx"])
    assert np.array_equal(r32["actions"].argmax(-1), r64["actions"].argmax(-1)) or not c.discrete


@pytest.mark.parametrize("name", IMAG_IDS)
def test_imag_float32_oracle_passes(name):
    c = sm.IMAG[name]
    err = sm.compare_imag(sm.run_oracle_imag(c, F32), sm.run_oracle_imag(c, F64), c.discrete, name)
    print(name, err)
    assert err["deter_abs"] < 1e-5 and err["actions_abs"] < 1e-5


@pytest.mark.parametrize("mut", ["wrong_block", "zero_initial", "row_offset_dropped"])
@pytest.mark.parametrize("name", IMAG_IDS)
def test_imag_comparison_fails_on_wrong_oracle(name, mut):
    c = sm.IMAG[name]
    cls = {"wrong_block": WrongBlock, "zero_initial": ZeroInitial, "row_offset_dropped": RowOffsetDropped}[mut]
    wrong = sm.run_oracle_imag(c, F32, cls=cls)
    with pytest.raises(AssertionError):
        sm.compare_imag(wrong, sm.run_oracle_imag(c, F64), c.discrete, f"{name} {mut}")


# --------------------------------------------------------------------------------------------------- the C gate
@pytest.mark.parametrize("D,G", [(256, 8), (768, 8), (160, 1), (96, 3)])  # Dg = 32, 96, 160, 32
def test_imagine_gate_refuses_blocks_that_are_no_multiple_of_64(D, G):
    """k_hid's 64-column tiles: Dg = 32 has no tile per block (a division by zero on the device), Dg = 96 or 160
    would straddle two blocks. The library says so when asked for the workspace, before any pointer exists."""
    from sdreamer import _native as nat
    assert sm.imagine_work_status(D, G, 4, 16) == nat.SD_ESHAPE


def test_imagine_gate_admits_the_fused_cases_only():
    from sdreamer import _native as nat
    for c in sm.IMAG_CASES:
        n = sm.imagine_work_status(c.D, c.G, c.S, c.K, c.A, c.discrete, c.actor_layers, c.img_layers, c.N, c.H1)
        assert (n > 0) if c.fused else (n == nat.SD_ESHAPE), (c.name, n)
    for bad in (dict(K=64), dict(S=3, K=16), dict(A=17), dict(A=17, discrete=True), dict(actor_layers=5),
                dict(img_layers=0), dict(D=8192, G=8)):
        kw = dict(D=512, G=8, S=4, K=16)
        kw.update(bad)
        assert sm.imagine_work_status(**kw) == nat.SD_ESHAPE, bad
