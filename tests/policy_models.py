"""Small acting cases for pinning the fused acting step (csrc/policy.hip, Dreamer.policy_step) to the float64 oracle
(oracle/ref_cpu.py Oracle.act) at every kind of shape its gate admits, and two shapes outside it. Test infrastructure
(a plain module: no fixtures, no pytest hooks), built on tests/small_models.py: dmc/proprio observations (the encoder
is the small MLP), parameters from oracle/init.py params_for(case seed), inputs from the case seed.

| name          | D    | G | S  | K  | B  | A        | layers | is_first   | seed | reaches                               |
|---------------|------|---|----|----|----|----------|--------|------------|------|---------------------------------------|
| b1_first      | 256  | 1 | 16 | 32 | 1  | 6 cont   | 3      | 1          | 0    | one row, one block, reset             |
| b1_carry      | 256  | 1 | 16 | 32 | 1  | 6 cont   | 3      | 0          | 0    | the carried state read                |
| b5_a16        | 512  | 2 | 32 | 16 | 5  | 16 cont  | 2      | rows 0, 3  | 0    | ragged tile, widest continuous head   |
| b17_onehot16  | 1024 | 2 | 32 | 32 | 17 | 16 disc  | 1      | r % 3 == 0 | 0    | two row tiles, SK 1024, Dg 512, one layer |
| anchor_a1     | 2048 | 8 | 32 | 16 | 16 | 1 cont   | 4      | r % 4 == 1 | 0    | the shipped size, A = 1, four layers  |
| out_kd64      | 1024 | 4 | 8  | 64 | 3  | 6 cont   | 3      | row 0      | 0    | scan admits, policy gate refuses      |
| out_dg96      | 768  | 8 | 4  | 16 | 3  | 6 cont   | 3      | row 0      | 0    | outside both                          |

seed: the first of 0, 1, 2, ... at which the case meets the input condition (tests/test_policy_parity_cpu.py: every
categorical's top-two margin under the float32 oracle >= small_models.MIN_MARGIN, float32 and float64 oracles draw the
same indices), chosen on the CPU from the oracle alone. Every case runs in both eval modes at ACT_STEP and ACT_SEED
(test_gpu_act.test_act_matches_oracle's). Index rule: exact equality. Tolerances: small_models' caps for the same
quantities (STATE_* for deter and the posterior logits, IMAG_* for continuous actions).
"""
import ctypes
import functools
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

import small_models as sm
from oracle import noise as nz
from oracle import ref_cpu
from oracle.ref_cpu import Oracle
from parity import perturbed_margin

ACT_SEED, ACT_STEP = 321, 4


@dataclass(frozen=True)
class PolicyCase:
    name: str
    D: int
    G: int
    S: int
    K: int
    B: int
    A: int
    discrete: bool
    actor_layers: int
    first: tuple  # the rows whose is_first is set
    admitted: bool  # sd_policy_step_ok / Dreamer._fused_policy_ok
    seed: int
    img_layers: int = 2  # (small_models.overrides reads it; acting does not run img_net)

    @property
    def Dg(self):
        return self.D // self.G


CASES = [
    PolicyCase("b1_first", 256, 1, 16, 32, 1, 6, False, 3, (0,), True, seed=0),
    PolicyCase("b1_carry", 256, 1, 16, 32, 1, 6, False, 3, (), True, seed=0),
    PolicyCase("b5_a16", 512, 2, 32, 16, 5, 16, False, 2, (0, 3), True, seed=0),
    PolicyCase("b17_onehot16", 1024, 2, 32, 32, 17, 16, True, 1, tuple(range(0, 17, 3)), True, seed=0),
    PolicyCase("anchor_a1", 2048, 8, 32, 16, 16, 1, False, 4, tuple(range(1, 16, 4)), True, seed=0),
    PolicyCase("out_kd64", 1024, 4, 8, 64, 3, 6, False, 3, (0,), False, seed=0),
    PolicyCase("out_dg96", 768, 8, 4, 16, 3, 6, False, 3, (0,), False, seed=0),
]
CASE = {c.name: c for c in CASES}
ADMITTED = [c for c in CASES if c.admitted]


@functools.lru_cache(maxsize=None)
def policy_inputs(c):
    """obs (position, velocity, is_first) and the carried state (one-hot stoch, deter, prev_action with |a| > 1
    included: action_norm's clip); CPU float32."""
    g = torch.Generator().manual_seed(100 + c.seed)
    obs = {k: torch.randn(c.B, *shp, generator=g) for k, shp in sm.OBS.items()}
    obs["is_first"] = torch.tensor([r in c.first for r in range(c.B)])
    idx = torch.randint(0, c.K, (c.B, c.S), generator=g)
    if c.discrete:
        a = F.one_hot(torch.randint(0, c.A, (c.B,), generator=g), c.A).float()
    else:
        a = 0.8 * torch.randn(c.B, c.A, generator=g)
    state = {"stoch": F.one_hot(idx, c.K).float(), "deter": 0.3 * torch.randn(c.B, c.D, generator=g), "prev_action": a}
    return obs, state


class PolicyOracle(Oracle):
    """Oracle.act restated with a row offset for the noise counters and the logits kept (act_ro(row_offset=0) equals
    Oracle.act bit for bit: test_policy_parity_cpu.test_restatement_is_oracle_act), plus the planted faults of the CPU
    self-check as switches."""
    no_reset = swap_streams = no_step = no_row_offset = eval_samples = scale_from_mean = False

    @torch.no_grad()
    def act_ro(self, obs, state, seed, step=0, eval=False, row_offset=0):
        s, DT = self.s, ref_cpu.DT
        embed = self.encode({k: v.unsqueeze(1) for k, v in obs.items() if k != "is_first"})[:, 0]
        B = embed.shape[0]
        rs = obs["is_first"].reshape(B)
        if self.no_reset:
            rs = torch.zeros_like(rs)
        stoch = torch.where(rs.reshape(B, 1, 1), torch.zeros_like(state["stoch"]), state["stoch"])
        deter = torch.where(rs.reshape(B, 1), torch.zeros_like(state["deter"]), state["deter"])
        act = torch.where(rs.reshape(B, 1), torch.zeros_like(state["prev_action"]), state["prev_action"])
        deter = self.deter_step(stoch, deter, act)
        logit = self.obs_logit(deter, embed)
        sp, sa = (nz.STREAM_POLICY_ACT, nz.STREAM_POLICY) if self.swap_streams else (nz.STREAM_POLICY, nz.STREAM_POLICY_ACT)
        step = 0 if self.no_step else step
        ro = 0 if self.no_row_offset else row_offset
        g = torch.from_numpy(nz.gumbel_block(seed, sp, step, B, ro, s.SK)).reshape(B, s.S, s.K)
        stoch = self.sample_stoch(logit, g)
        logits = self.head_logits("actor", self.get_feat(stoch, deter))
        if self.scale_from_mean and not s.discrete:
            logits = torch.cat([logits[:, :s.A], logits[:, :s.A]], -1)
        if eval and not self.eval_samples:
            action = F.one_hot(logits.argmax(-1), s.A).to(DT) if s.discrete else torch.tanh(logits[:, :s.A])
        else:
            action = self.actor_sample(logits, seed, step, ro, sa)
        return action, {"stoch": stoch, "deter": deter, "prev_action": action}, logit, logits


def oracle_for(c, dtype, params=None, **mut):
    """PolicyOracle of a case in `dtype` (params: another parameter table, reference names, numpy)."""
    spec, p0 = sm.spec_params(c)
    P = {k: torch.tensor(v, dtype=dtype) for k, v in (params or p0).items()
         if k.startswith(("rssm.", "actor.", "encoder."))}
    orc = PolicyOracle(spec, P)
    for k, v in mut.items():
        setattr(orc, k, v)
    return orc


def _cast(d, dtype):
    return {k: (v if v.dtype == torch.bool else v.to(dtype)) for k, v in d.items()}


def pack(c, action, state, logit=None, alogit=None):
    f64 = lambda t: None if t is None else t.detach().cpu().numpy().astype(np.float64)  # noqa: E731
    return dict(idx=state["stoch"].reshape(-1, c.S, c.K).argmax(-1).cpu().numpy(),
                deter=f64(state["deter"]), action=f64(action),
                logit=f64(None if logit is None else logit.reshape(-1, c.S, c.K)), actor_logit=f64(alogit))


def run_oracle(c, dtype=torch.float64, eval=False, row_offset=0, rows=None, state=None, params=None, **mut):
    """rows: run on these rows of the case's inputs only (the row-offset test). state: another carried state."""
    if not mut and rows is None and state is None and params is None:
        return _run_oracle_cached(c, dtype, bool(eval), int(row_offset))
    return _run_oracle(c, dtype, eval, row_offset, rows, state, params, mut)


@functools.lru_cache(maxsize=None)
def _run_oracle_cached(c, dtype, eval, row_offset):
    return _run_oracle(c, dtype, eval, row_offset, None, None, None, {})


def _run_oracle(c, dtype, eval, row_offset, rows, state, params, mut):
    obs, st0 = policy_inputs(c)
    st0 = state or st0
    if rows is not None:
        obs, st0 = {k: v[rows] for k, v in obs.items()}, {k: v[rows] for k, v in st0.items()}
    with sm.oracle_dtype(dtype):
        a, st, logit, alogit = oracle_for(c, dtype, params, **mut).act_ro(
            _cast(obs, dtype), _cast(st0, dtype), ACT_SEED, ACT_STEP, eval, row_offset)
    return pack(c, a, st, logit, alogit)


def run_product(ag, c, eval=False, row_offset=0, rows=None, state=None, fn="policy_step"):
    """Dreamer.policy_step (or act) on the case's inputs -> the packed result and the raw device tensors"""
    obs, st0 = policy_inputs(c)
    st0 = state or st0
    if rows is not None:
        obs, st0 = {k: v[rows] for k, v in obs.items()}, {k: v[rows] for k, v in st0.items()}
    obs, st0 = {k: v.cuda() for k, v in obs.items()}, {k: v.cuda() for k, v in st0.items()}
    kw = dict(row_offset=row_offset) if fn == "policy_step" else {}
    a, st = getattr(ag, fn)(obs, st0, eval=eval, seed=ACT_SEED, step=ACT_STEP, **kw)
    torch.cuda.synchronize()
    out = pack(c, a, st)
    out["raw"] = (a.clone(), {k: v.clone() for k, v in st.items()})
    return out


# --------------------------------------------------------------------------------------------------- margins
def min_margin(c, ref32, eval, row_offset=0):
    """smallest top-two margin over the posterior categoricals and, for a one-hot actor with a choice, the action (the
    Gumbel-perturbed unimix logits when sampled, the raw logits for the mode)"""
    spec, _ = sm.spec_params(c)
    B = ref32["logit"].shape[0]
    g = nz.gumbel_block(ACT_SEED, nz.STREAM_POLICY, ACT_STEP, B, row_offset, c.S * c.K).reshape(B, c.S, c.K)
    m = float(perturbed_margin(ref32["logit"], g, spec.unimix).min())
    if c.discrete and c.A > 1:
        al = ref32["actor_logit"]
        if eval:
            top = np.sort(al, -1)
            m = min(m, float((top[:, -1] - top[:, -2]).min()))
        else:
            ga = nz.gumbel_block(ACT_SEED, nz.STREAM_POLICY_ACT, ACT_STEP, B, row_offset, c.A)
            m = min(m, float(perturbed_margin(al, ga, float(spec.actor_dist.unimix_ratio)).min()))
    return m


# --------------------------------------------------------------------------------------------------- comparisons
def policy_errors(got, ref, discrete):
    assert got["idx"].shape == ref["idx"].shape and got["action"].shape == ref["action"].shape
    out = dict(idx_mismatch=int((got["idx"] != ref["idx"]).sum()), act_mismatch=0, action_ratio=0.0)
    out["deter_ratio"] = sm._ratio(got["deter"], ref["deter"], sm.STATE_RTOL, sm.STATE_ATOL)
    if got.get("logit") is not None:
        out["logit_ratio"] = sm._ratio(got["logit"], ref["logit"], sm.STATE_RTOL, sm.STATE_ATOL)
    if discrete:
        out["act_mismatch"] = int((got["action"].argmax(-1) != ref["action"].argmax(-1)).sum())
        out["act_mismatch"] += int((np.abs(got["action"] - ref["action"]) > sm.IMAG_ATOL).sum())
    else:
        out["action_ratio"] = sm._ratio(got["action"], ref["action"], sm.IMAG_RTOL, sm.IMAG_ATOL)
    return out


def policy_failures(got, ref, discrete):
    err = policy_errors(got, ref, discrete)
    bad = []
    if err["idx_mismatch"]:
        bad.append(f"{err['idx_mismatch']} posterior indices differ")
    if err["act_mismatch"]:
        bad.append(f"{err['act_mismatch']} one-hot action elements differ")
    for k in ("deter_ratio", "logit_ratio", "action_ratio"):
        if k in err and not err[k] <= 1.0:
            bad.append(f"{k[:-6]} uses {err[k]:.3g} of its bound")
    return bad, err


def compare_policy(got, ref, discrete, what=""):
    bad, err = policy_failures(got, ref, discrete)
    assert not bad, f"{what}: " + "; ".join(bad)
    return err


# --------------------------------------------------------------------------------------------------- the C gate
def desc(D, G, S, K, B=3, A=6, discrete=False, actor_layers=3, U=256, E=256):
    """sd_policy of these shapes and no pointers (host only)"""
    from sdreamer import _native as nat
    d = nat.PolicyDesc()
    d.B, d.D, d.U, d.SK, d.Kd, d.G, d.A, d.E = B, D, U, S * K, K, G, A, E
    d.act_discrete, d.actor_layers = int(discrete), actor_layers
    return d


def case_desc(c):
    spec, _ = sm.spec_params(c)
    return desc(c.D, c.G, c.S, c.K, c.B, c.A, c.discrete, c.actor_layers, E=spec.E)


def c_ok(d):
    from sdreamer import _native as nat
    return nat.fns["sd_policy_step_ok"](ctypes.addressof(d))
