"""The acting cases (tests/policy_models.py) on the CPU: the input condition that lets the GPU tests demand exact
indices, the float32 oracle against the float64 oracle under the GPU tests' caps, planted faults that the comparison
must catch, and the host side of sd_policy_step (descriptor layout, shape gate, agreement with the Python gate)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import policy_models as pm
import small_models as sm
from oracle.ref_cpu import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sdhip.h")
MODES = [False, True]


@pytest.mark.parametrize("ev", MODES)
@pytest.mark.parametrize("c", pm.ADMITTED, ids=lambda c: c.name)
def test_input_condition(c, ev):
    """every categorical's top-two margin under the float32 oracle >= MIN_MARGIN; float32 and float64 draw the same"""
    r32, r64 = pm.run_oracle(c, torch.float32, ev), pm.run_oracle(c, torch.float64, ev)
    m = pm.min_margin(c, r32, ev)
    print(f"{c.name} eval={ev}: min margin {m:.3g}")
    assert m >= sm.MIN_MARGIN, f"{c.name}: margin {m:.3g}: take the next seed"
    assert np.array_equal(r32["idx"], r64["idx"])
    if c.discrete:
        assert np.array_equal(r32["action"].argmax(-1), r64["action"].argmax(-1))


@pytest.mark.parametrize("ev", MODES)
@pytest.mark.parametrize("c", pm.ADMITTED, ids=lambda c: c.name)
def test_float32_oracle_within_caps(c, ev):
    err = pm.compare_policy(pm.run_oracle(c, torch.float32, ev), pm.run_oracle(c, torch.float64, ev), c.discrete, c.name)
    print(c.name, ev, err)


@pytest.mark.parametrize("c", pm.CASES, ids=lambda c: c.name)
def test_restatement_is_oracle_act(c):
    """PolicyOracle.act_ro at row offset 0 is Oracle.act, bit for bit (both modes)"""
    obs, st = pm.policy_inputs(c)
    spec, params = sm.spec_params(c)
    P = {k: torch.from_numpy(v) for k, v in params.items()}
    for ev in MODES:
        a0, s0 = Oracle(spec, P).act(obs, st, pm.ACT_SEED, pm.ACT_STEP, ev)
        a1, s1, _, _ = pm.PolicyOracle(spec, P).act_ro(obs, st, pm.ACT_SEED, pm.ACT_STEP, ev)
        assert torch.equal(a0, a1) and all(torch.equal(s0[k], s1[k]) for k in s0)


FAULTS = ["no_reset", "swap_streams", "no_step", "no_row_offset", "eval_samples", "scale_from_mean"]


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_is_caught(fault):
    """each mutated float64 oracle fails the comparison with the right one on at least one case (row_offset 3 for the
    fault that ignores it; the others at the cases' own row offset 0)"""
    ro = 3 if fault == "no_row_offset" else 0
    caught = []
    for c in pm.ADMITTED:
        for ev in MODES:
            ref = pm.run_oracle(c, torch.float64, ev, ro)
            bad, _ = pm.policy_failures(pm.run_oracle(c, torch.float64, ev, ro, **{fault: True}), ref, c.discrete)
            if bad:
                caught.append((c.name, ev))
    print(fault, caught)
    assert caught, f"{fault}: no case fails"


PROBE = ["B", "actor_layers", "eps", "max_std", "eval", "seed", "seed_ptr", "step", "row_offset", "stream_act", "W0",
         "n2", "Wg", "Wo", "Wl", "Wa", "na", "Wao", "embed", "is_first", "prev_action", "stoch_out", "actor_logit", "work"]


def test_desc_layout_matches_c():
    from sdreamer import _native as nat
    S, cname = nat.PolicyDesc, "sd_policy"
    assert S._fields_[0][0] == PROBE[0] and S._fields_[-1][0] == PROBE[-1]
    fmt = " ".join(["%zu"] * (len(PROBE) + 1))
    args = ", ".join([f"sizeof({cname})"] + [f"offsetof({cname}, {f})" for f in PROBE])
    src = f'#include <stdio.h>\n#include <stddef.h>\n#include "sdhip.h"\nint main(void){{printf("{fmt}", {args}); return 0;}}\n'
    with tempfile.TemporaryDirectory() as d:
        cfile = os.path.join(d, "t.c")
        open(cfile, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.dirname(HEADER), cfile, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in PROBE]


def test_gate_on_host_only_descriptors():
    """no pointer is set: the gate reads shapes only, launches nothing and touches no device"""
    from sdreamer import _native as nat
    ok, floats, run = (nat.fns[n] for n in ("sd_policy_step_ok", "sd_policy_step_work_floats", "sd_policy_step"))
    good = pm.desc(2048, 8, 32, 16, B=16)
    assert ok(ctypes.addressof(good)) == 1 and floats(ctypes.addressof(good)) > 0
    assert run(ctypes.addressof(good), 0) == -1  # SD_EARG: admitted shape, null pointers; refused before any launch
    bads = [pm.case_desc(pm.CASE["out_kd64"]), pm.case_desc(pm.CASE["out_dg96"]), pm.desc(2048, 8, 32, 16, U=128),
            pm.desc(2048, 8, 32, 16, A=17, discrete=True), pm.desc(2048, 8, 32, 16, actor_layers=5),
            pm.desc(2048, 8, 32, 16, B=0), pm.desc(2048, 8, 32, 16, B=4097), pm.desc(2048, 8, 32, 16, A=17),
            pm.desc(2048, 8, 32, 16, E=0), pm.desc(2048, 8, 32, 16, E=250)]
    for bad in bads:
        assert ok(ctypes.addressof(bad)) == 0
        assert floats(ctypes.addressof(bad)) == nat.SD_ESHAPE
        assert run(ctypes.addressof(bad), 0) == nat.SD_ESHAPE
    assert ok(0) == 0
    for c in pm.CASES:
        assert (pm.c_ok(pm.case_desc(c)) == 1) == c.admitted, c.name


class _Stub:
    """the attributes Dreamer._fused_policy_ok reads, from a case (no device, no parameters)"""

    def __init__(self, c, E):
        ns = lambda **kw: type("NS", (), kw)()  # noqa: E731
        self.rssm = ns(_deter=c.D, _blocks=c.G, flat_stoch=c.S * c.K, _discrete=c.K, _hidden=256, embed_size=E)
        self.actor = ns(mlp=ns(_symlog_inputs=False, out_dim=256, n=c.actor_layers),
                        dist_name="onehot" if c.discrete else "bounded_normal")
        self.act_dim, self.act_discrete = c.A, c.discrete


@pytest.mark.parametrize("c", pm.CASES, ids=lambda c: c.name)
def test_python_gate_agrees_with_c(c):
    from sdreamer.dreamer import Dreamer
    spec, _ = sm.spec_params(c)
    got = Dreamer._fused_policy_ok(_Stub(c, spec.E), c.B)
    assert got == (pm.c_ok(pm.case_desc(c)) == 1) == c.admitted
    # and what the C gate cannot see: a symlog-input actor, another distribution
    st = _Stub(c, spec.E)
    st.actor.mlp._symlog_inputs = True
    assert not Dreamer._fused_policy_ok(st, c.B)
    st = _Stub(c, spec.E)
    st.actor.dist_name = "multi_discrete"
    assert not Dreamer._fused_policy_ok(st, c.B)
