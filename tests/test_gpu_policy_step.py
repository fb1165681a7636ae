"""Dreamer.policy_step / sd_policy_step (csrc/policy.hip: acting after the encoder as 5 + actor-layers fused launches)
against the float64 oracle at every case of tests/policy_models.py, and the properties around it: the C entry on raw
buffers, the reset select, the row offset, parameters changed between calls, the launch route, graph replay, and that
act / update_batch launch what they launched before. Index rule: exact (the input condition is enforced on the CPU,
tests/test_policy_parity_cpu.py); tolerances: small_models' caps."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import policy_models as pm
import small_models as sm
from launch_trace import recorded

pytestmark = pytest.mark.gpu
MODES = [False, True]
PER_OP = ("sd_mask_rows", "sd_action_norm", "sd_gru_fwd", "sd_onehot_sample_fwd", "sd_bnormal_sample", "sd_rmsnorm_fwd")


@functools.lru_cache(maxsize=None)
def agent(name):
    return sm.build_product(pm.CASE[name])


@pytest.mark.parametrize("ev", MODES)
@pytest.mark.parametrize("c", pm.ADMITTED, ids=lambda c: c.name)
def test_policy_step_matches_float64_oracle(c, ev):
    got = pm.run_product(agent(c.name), c, ev)
    err = pm.compare_policy(got, pm.run_oracle(c, torch.float64, ev), c.discrete, f"{c.name} eval={ev}")
    print(c.name, ev, err)


def _raw_call(ag, c, ev, want_logits):
    """sd_policy_step on buffers of the test's own (the embed from the product's encoder, as policy_step forms it)"""
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    from sdreamer.rssm import STREAM_POLICY, STREAM_POLICY_ACT
    obs, st = pm.policy_inputs(c)
    obs, st = {k: v.cuda() for k, v in obs.items()}, {k: v.cuda() for k, v in st.items()}
    with torch.no_grad():
        embed = ag.encoder({k: v.unsqueeze(1) for k, v in obs.items() if k != "is_first"})[:, 0].contiguous()
    d, keep = ag._policy_desc(c.B)
    d.eval, d.step, d.row_offset, d.seed = int(ev), pm.ACT_STEP, 0, pm.ACT_SEED
    d.stream_post, d.stream_act = STREAM_POLICY, STREAM_POLICY_ACT
    NO = c.A if c.discrete else 2 * c.A
    e = lambda *s: torch.full(s, float("nan"), device="cuda")  # noqa: E731
    outs = dict(stoch_out=e(c.B, c.S * c.K), deter_out=e(c.B, c.D), action=e(c.B, c.A))
    if want_logits:
        outs.update(logit=e(c.B, c.S * c.K), actor_logit=e(c.B, NO))
    ins = dict(embed=embed, is_first=obs["is_first"].to(torch.uint8), stoch=st["stoch"].reshape(c.B, -1).contiguous(),
               deter=st["deter"], prev_action=st["prev_action"])
    for k, v in {**ins, **outs}.items():
        setattr(d, k, v.data_ptr())
    n = nat.fns["sd_policy_step_work_floats"](ctypes.addressof(d))
    assert n > 0
    work = e(n)
    d.work = work.data_ptr()
    nat.call("sd_policy_step", ctypes.addressof(d), K.stream())
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("ev", MODES)
def test_c_entry_on_raw_buffers(ev):
    """the entry called directly gives policy_step's bits, with and without the optional logits, which match the
    oracle's; the workspace arrives filled with NaN (nothing is read before it is written)"""
    c = pm.CASE["b5_a16"]
    ag = agent(c.name)
    a, st = pm.run_product(ag, c, ev)["raw"]
    ref = pm.run_oracle(c, torch.float64, ev)
    for want in (True, False):
        o = _raw_call(ag, c, ev, want)
        assert torch.equal(o["action"], a) and torch.equal(o["deter_out"], st["deter"])
        assert torch.equal(o["stoch_out"].view(c.B, c.S, c.K), st["stoch"])
        if want:
            r = sm._ratio(o["logit"].view(c.B, c.S, c.K).cpu().numpy().astype(np.float64), ref["logit"], sm.STATE_RTOL,
                          sm.STATE_ATOL)
            ra = sm._ratio(o["actor_logit"].cpu().numpy().astype(np.float64), ref["actor_logit"], sm.IMAG_RTOL,
                           sm.IMAG_ATOL)
            print(f"logit uses {r:.3g}, actor logit {ra:.3g} of the bound")
            assert r <= 1.0 and ra <= 1.0


@pytest.mark.parametrize("ev", MODES)
def test_reset_rows_ignore_the_carried_state(ev):
    """what the caller left in the is_first rows (zeros, or 1e30) does not reach any output: a select, not a multiply"""
    c = pm.CASE["b17_onehot16"]
    obs, st = pm.policy_inputs(c)
    outs = []
    for fill in (0.0, 1e30):
        s2 = {k: v.clone() for k, v in st.items()}
        for k in s2:
            s2[k][obs["is_first"]] = fill
        outs.append(pm.run_product(agent(c.name), c, ev, state=s2)["raw"])
    (a0, s0), (a1, s1) = outs
    assert torch.equal(a0, a1) and all(torch.equal(s0[k], s1[k]) for k in s0)
    assert torch.isfinite(a1).all() and torch.isfinite(s1["deter"]).all()


@pytest.mark.parametrize("ev", MODES)
def test_row_offset_selects_the_noise_rows(ev):
    """rows 3..5 at row_offset 0 against a B = 3 call on the same rows at row_offset 3: the same draws"""
    c = pm.CASE["b17_onehot16"]
    ag = agent(c.name)
    full = pm.run_product(ag, c, ev)
    rows = slice(3, 6)
    part = pm.run_product(ag, c, ev, row_offset=3, rows=rows)
    sub = {k: (None if full[k] is None else full[k][rows]) for k in ("idx", "deter", "action", "logit", "actor_logit")}
    pm.compare_policy(part, sub, c.discrete, "rows 3..5")
    pm.compare_policy(part, pm.run_oracle(c, torch.float64, ev, 3, rows=rows), c.discrete, "rows 3..5 against float64")


def test_parameters_changed_between_calls_are_seen():
    """no weight image outlives a call: 0.05 added in place to the actor's last weight and to _dyn_in0's norm weight"""
    c = pm.CASE["b1_carry"]
    ag = agent(c.name)
    names = ("actor.last.weight", "rssm._deter_net._dyn_in0.1.weight")
    ps = dict(ag.named_parameters())
    saved = {n: ps[n].detach().clone() for n in names}
    try:
        first = pm.run_product(ag, c, False)
        pm.compare_policy(first, pm.run_oracle(c, torch.float64, False), c.discrete, "before")
        _, params = sm.spec_params(c)
        changed = dict(params)
        with torch.no_grad():
            for n in names:
                ps[n].add_(0.05)
                changed[n] = params[n] + np.float32(0.05)
        second = pm.run_product(ag, c, False)
        pm.compare_policy(second, pm.run_oracle(c, torch.float64, False, params=changed), c.discrete, "after")
        assert not np.array_equal(first["action"], second["action"])
        assert not np.array_equal(first["deter"], second["deter"])
    finally:
        with torch.no_grad():
            for n in names:
                ps[n].copy_(saved[n])


@pytest.mark.parametrize("c", pm.CASES, ids=lambda c: c.name)
def test_route(c):
    """admitted: the launches are the encoder's own (recorded alone: the small MLP encoder runs sd_rmsnorm_fwd itself, so
    "no per-op name anywhere" cannot hold) followed by exactly one sd_policy_step and nothing else, so none of the
    per-op acting entries follows the encoder; outside the gate: act's launches and act's bits"""
    ag = agent(c.name)
    got, names = recorded(lambda: pm.run_product(ag, c, False))
    if c.admitted:
        obs = {k: v.cuda().unsqueeze(1) for k, v in pm.policy_inputs(c)[0].items() if k != "is_first"}
        with torch.no_grad():
            _, enc = recorded(lambda: ag.encoder(obs))
        assert names.count("sd_policy_step") == 1, names
        assert names == enc + ["sd_policy_step"], names
        assert not [n for n in names[len(enc):] if n in PER_OP], names
    else:
        assert "sd_policy_step" not in names
        a, st = pm.run_product(ag, c, False, fn="act")["raw"]
        assert torch.equal(got["raw"][0], a) and all(torch.equal(got["raw"][1][k], st[k]) for k in st)


def test_fused_policy_graph_equals_eager_policy_step():
    """three replays equal eager policy_step(seed = base + k) bit for bit (is_first set on the first call only); the
    per-op policy_graph still equals act in the same process"""
    c = pm.CASE["b5_a16"]
    ag = agent(c.name)
    obs, state = pm.policy_inputs(c)
    obs, state = {k: v.cuda() for k, v in obs.items()}, {k: v.cuda() for k, v in state.items()}
    base = ag._seed_base + 7
    for fused, eager in ((True, ag.policy_step), (False, ag.act)):
        o = dict(obs)
        policy = ag.policy_graph(c.B, o, fused=fused) if fused else ag.policy_graph(c.B, o)
        st_g, st_e = dict(state), dict(state)
        for k in range(3):
            a_g, st_g = policy(o, st_g)
            a_g, st_g = a_g.clone(), {n: v.clone() for n, v in st_g.items()}
            a_e, st_e = eager(o, st_e, seed=base + k, step=0)
            assert torch.equal(a_g, a_e), (fused, k)
            for n in st_e:
                assert torch.equal(st_g[n], st_e[n]), (fused, k, n)
            o["is_first"] = torch.zeros_like(o["is_first"])


def _golden_inputs(name, B, seed):
    from test_gpu_act import _inputs
    from test_gpu_dreamer import build_agent
    ag, z, spec, obs_shapes = build_agent(name)
    A, discrete = int(z["meta_A"]), bool(z["meta_discrete"])
    obs, state = _inputs(spec, obs_shapes, B, A, discrete, seed)
    return ag, z, spec, (discrete, obs_shapes), {k: v.cuda() for k, v in obs.items()}, \
        {k: v.cuda() for k, v in state.items()}


def test_act_and_update_launch_what_they_launched():
    """the launch-name sequences of act and of one update_batch on the walker_r2 golden agent, before and after one
    policy_step on that agent"""
    from golden_io import batch, initial
    ag, z, spec, (_, obs_shapes), obs, state = _golden_inputs("walker_r2", 6, 5)
    ag.use_graphs = False
    data, init = batch(z, 0, obs_shapes, "cuda:0"), initial(z, 0, spec, "cuda:0")
    ag.update_batch(data, init, 11)  # warm-up: one-time work (buffers, cached layouts) is done
    _, upd0 = recorded(lambda: ag.update_batch(data, init, 12))
    _, act0 = recorded(lambda: ag.act(obs, state, seed=321, step=4))
    _, names = recorded(lambda: ag.policy_step(obs, state, seed=321, step=4))
    assert names.count("sd_policy_step") == 1
    _, upd1 = recorded(lambda: ag.update_batch(data, init, 13))
    _, act1 = recorded(lambda: ag.act(obs, state, seed=321, step=4))
    assert act0 == act1 and "sd_policy_step" not in act0
    assert upd0 == upd1 and "sd_policy_step" not in upd0


@pytest.mark.parametrize("name", ["walker_r2", "atari_r2"])
@pytest.mark.parametrize("ev", MODES)
def test_policy_step_against_act_on_golden_agents(name, ev):
    """Both golden agents are admitted (D 2048, G 8, SK 512 / 1024, Kd 16 / 32, E 1024, three actor layers; walker: 6
    continuous actions, atari: 4 discrete): the posterior indices are act's, deter and continuous actions within 1e-4
    abs, discrete actions equal."""
    ag, z, spec, (discrete, _), obs, state = _golden_inputs(name, 6, 5)
    assert ag._fused_policy_ok(6)
    a0, s0 = ag.act(obs, state, eval=ev, seed=321, step=4)
    a1, s1 = ag.policy_step(obs, state, eval=ev, seed=321, step=4)
    torch.cuda.synchronize()
    assert torch.equal(s1["stoch"].argmax(-1), s0["stoch"].argmax(-1))
    print(name, ev, "deter", float((s1["deter"] - s0["deter"]).abs().max()), "action", float((a1 - a0).abs().max()))
    np.testing.assert_allclose(s1["deter"].cpu().numpy(), s0["deter"].cpu().numpy(), atol=1e-4, rtol=0)
    if discrete:
        assert torch.equal(a1, a0)
    else:
        np.testing.assert_allclose(a1.cpu().numpy(), a0.cpu().numpy(), atol=1e-4, rtol=0)
