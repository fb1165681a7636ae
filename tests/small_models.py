"""Small RSSM / imagination cases for pinning the fused kernels (csrc/scan.hip, csrc/img.hip) and their per-op
fallbacks to the float64 oracle (oracle/ref_cpu.py with ref_cpu.DT = torch.float64) at every kind of shape the gates
admit, not only the three BASELINE model sizes. Test infrastructure (a plain module: no fixtures, no pytest hooks).

Shared by tests/test_small_model_parity_cpu.py (the input condition, float32 oracle against float64, mutated
oracles), tests/test_gpu_scan_f64.py and tests/test_gpu_imagine_f64.py (the product against float64). Everything is
regenerated from each case's seed: parameters (oracle/init.py params_for), inputs and the Philox noise seed.

Index rule here: EXACT equality, no near-tie allowance. The CPU file enforces, per case, that every categorical's
top-2 perturbed-logit margin under the float32 oracle is >= MIN_MARGIN (ten times parity.MARGIN) and that the float32
and float64 oracles draw the same indices; a case that fails gets another seed (chosen on the CPU, from the oracle
alone). Tolerances are the project's (test_gpu_scan.py, test_gpu_imagine.py), used as caps.
"""
import contextlib
import copy
import ctypes
import functools
from dataclasses import dataclass

import numpy as np
import torch

from oracle import noise as nz
from oracle import ref_cpu
from oracle.init import params_for
from oracle.ref_cpu import Oracle, Spec
from parity import imag_margins, perturbed_margin, post_margins
from sdreamer.config import load_config

CONFIG = "dmc/proprio"
OBS = {"position": (8,), "velocity": (9,)}
MIN_MARGIN = 1e-4  # 10 x parity.MARGIN
# caps (test_gpu_scan.py / test_gpu_imagine.py)
STATE_RTOL, STATE_ATOL = 1e-3, 1e-4  # scan forward deter / logits
GRAD_REL, GRAD_ABS = 2e-3, 1e-7  # scan gradients: of each tensor's max
IMAG_RTOL, IMAG_ATOL = 1e-3, 2e-4  # imagined deter / actions
IMAG_ROW_OFFSET = 3  # global row of the first imagined row (the noise counters' offset)


@dataclass(frozen=True)
class ScanCase:
    name: str
    D: int
    G: int
    S: int
    K: int
    B: int
    T: int
    fused: bool  # rssm._fused_scan_ok
    seed: int
    rot: int = 0  # row r takes reset pattern (r + rot) % 4, see scan_inputs
    A: int = 6
    discrete: bool = False
    actor_layers: int = 3
    img_layers: int = 2

    @property
    def Dg(self):
        return self.D // self.G


@dataclass(frozen=True)
class ImagCase:
    name: str
    D: int
    G: int
    S: int
    K: int
    A: int
    discrete: bool
    actor_layers: int
    img_layers: int
    N: int
    H1: int
    fused: bool  # Dreamer._fused_imag_ok
    plan: str  # the kernels csrc/img.hip iplan() picks by default at this shape ("per-op" outside the gate)
    seed: int

    @property
    def Dg(self):
        return self.D // self.G


# what each case reaches is in the test files' tables; seeds: the first of 0, 1, 2, ... that meets the input condition
SCAN_CASES = [
    ScanCase("t1_b1_init", 256, 1, 16, 32, 1, 1, True, seed=0),  # T = 1, one row, one block; stoch0 / deter0 read
    ScanCase("t1_b1_reset", 256, 1, 16, 32, 1, 1, True, seed=0, rot=1),  # the same shape, the row reset
    ScanCase("kd64_sk512", 1024, 4, 8, 64, 5, 3, True, seed=0),
    ScanCase("kd64_sk1024_b17", 1024, 2, 16, 64, 17, 3, True, seed=0),
    ScanCase("s64", 512, 2, 64, 16, 3, 4, True, seed=0),
    ScanCase("anchor", 2048, 8, 32, 16, 16, 4, True, seed=0),
    ScanCase("per_op_sk64", 512, 8, 4, 16, 3, 2, False, seed=0),
    ScanCase("per_op_dg96", 768, 8, 4, 16, 3, 2, False, seed=0),
]
IMAG_CASES = [
    ImagCase("dg64", 512, 8, 4, 16, 6, False, 3, 2, 65, 3, True, "k_hid<true> + k_lin6", seed=0),
    ImagCase("sk64_a16", 128, 2, 2, 32, 16, False, 1, 4, 1, 4, True, "k_hid<true> + k_lin6", seed=0),
    ImagCase("s68_onehot16", 256, 4, 68, 16, 16, True, 3, 2, 70, 3, True, "k_hid<false> + k_lin", seed=2),  # seeds 0, 1: a margin of 7e-5
    ImagCase("dg256_onehot1", 1024, 4, 32, 32, 1, True, 4, 1, 130, 3, True, "k_hid_areg + k_lin6", seed=0),
    ImagCase("areg_h2", 2048, 8, 32, 16, 1, False, 3, 2, 64, 2, True, "k_hid_areg + k_lin6_areg", seed=0),
    ImagCase("per_op_dg96", 768, 8, 4, 16, 6, False, 3, 2, 65, 3, False, "per-op", seed=0),
    ImagCase("per_op_dg32", 256, 8, 4, 16, 6, False, 3, 2, 65, 3, False, "per-op", seed=0),
]
SCAN = {c.name: c for c in SCAN_CASES}
IMAG = {c.name: c for c in IMAG_CASES}
GRAD_COMBOS = [("deter",), ("logit",), ("stoch", "deter")]  # upstream gradients present (the others are None)
ALL_GRADS = ("stoch", "deter", "logit")


def imag_plan(c):
    """csrc/img.hip icheck() / iplan() restated: which kernels a default sd_imagine_run launches at this shape."""
    if c.Dg % 64 or (c.S * c.K) % 64 or c.K not in (16, 32) or c.D > 4096:
        return "per-op"
    if c.S > 64:  # more categoricals than a wave has lanes: no pre-split activation images
        return "k_hid<false> + k_lin"
    hid = "k_hid_areg" if c.Dg in (256, 512) else "k_hid<true>"
    return hid + (" + k_lin6_areg" if c.D in (2048, 4096) else " + k_lin6")


def noise_seed(c):
    return 1000 + 77 * c.seed


def overrides(c):
    return [f"model.deter={c.D}", f"model.rssm.blocks={c.G}", f"model.rssm.stoch={c.S}", f"model.discrete={c.K}",
            f"model.actor.layers={c.actor_layers}", f"model.rssm.img_layers={c.img_layers}", "model.compile=False"]


@functools.lru_cache(maxsize=None)
def spec_params(c):
    """Spec and the deterministic parameters (reference names / layouts) of a case."""
    cfg = load_config(CONFIG, ["device=cpu"] + overrides(c))
    spec = Spec(cfg.model, OBS, c.A, c.discrete)
    assert spec.U == 256 and (spec.D, spec.G, spec.S, spec.K) == (c.D, c.G, c.S, c.K)
    return spec, params_for(spec.shapes, c.seed)


class _Sp:
    def __init__(self, shape):
        self.shape = tuple(shape)


class _Spaces:
    def __init__(self, d):
        self.spaces = d


def build_product(c):
    """The product Dreamer of a case with the case's parameters, loaded through load_state_dict (the checkpoint
    layout), as test_gpu_fullsize._run_product does."""
    from sdreamer.dreamer import Dreamer
    spec, params = spec_params(c)
    gcfg = load_config(CONFIG, ["device=cuda:0"] + overrides(c))
    act = _Sp((c.A,))
    if c.discrete:
        act.discrete = True
    ag = Dreamer(copy.deepcopy(gcfg.model), _Spaces({k: _Sp(v) for k, v in OBS.items()}), act)
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    for k, sk in spec.slow_names.items():
        sd[sk] = torch.from_numpy(params[k])
    sd["return_ema.ema_vals"] = torch.zeros(2)
    missing, unexpected = ag.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert not [m for m in missing if not m.startswith("_frozen")], missing
    return ag


@contextlib.contextmanager
def oracle_dtype(dtype):
    """The oracle's arithmetic type for the duration of the block (ref_cpu.DT is read at call time)."""
    old = ref_cpu.DT
    ref_cpu.DT = dtype
    try:
        yield
    finally:
        ref_cpu.DT = old


# --------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def scan_inputs(c):
    """embed, action, reset, (stoch0, deter0), upstream gradients of (post_stoch, post_deter, post_logit); CPU float32.
    Reset pattern of row r by (r + rot) % 4: 0 never reset (the nonzero initial state is read), 1 reset at every
    step, 2 reset at step T - 1 only, 3 random flags (step 0 included)."""
    spec, _ = spec_params(c)
    B, T, S, K, D = c.B, c.T, c.S, c.K, c.D
    g = torch.Generator().manual_seed(c.seed)
    embed = torch.randn(B, T, spec.E, generator=g)
    action = torch.randn(B, T, c.A, generator=g)  # |a| > 1 included: action_norm's clip
    reset = torch.rand(B, T, generator=g) < 0.3
    for r in range(B):
        mode = (r + c.rot) % 4
        if mode == 0:
            reset[r] = False
        elif mode == 1:
            reset[r] = True
        elif mode == 2:
            reset[r] = False
            reset[r, T - 1] = True
    idx = torch.randint(0, K, (B, S), generator=g)
    init = (torch.nn.functional.one_hot(idx, K).float(), 0.5 * torch.randn(B, D, generator=g))
    ups = dict(stoch=torch.randn(B, T, S, K, generator=g), deter=0.1 * torch.randn(B, T, D, generator=g),
               logit=0.1 * torch.randn(B, T, S, K, generator=g))
    return embed, action, reset, init, ups


@functools.lru_cache(maxsize=None)
def imag_inputs(c):
    """start state of the N imagined rows: one-hot stoch (N, S, K), deter 0.5 randn (N, D); CPU float32."""
    g = torch.Generator().manual_seed(c.seed)
    idx = torch.randint(0, c.K, (c.N, c.S), generator=g)
    return torch.nn.functional.one_hot(idx, c.K).float(), 0.5 * torch.randn(c.N, c.D, generator=g)


# --------------------------------------------------------------------------------------------------- oracle runs
def _oracle(c, dtype, cls, prefixes):
    spec, params = spec_params(c)
    P = {k: torch.tensor(v, dtype=dtype).requires_grad_(True) for k, v in params.items() if k.startswith(prefixes)}
    return cls(spec, P), P


def run_oracle_scan(c, dtype=torch.float64, grads=ALL_GRADS, cls=Oracle, **mut):
    """Oracle.observe forward and the autograd gradient of sum_k <output_k, upstream_k> over the outputs in `grads`.
    cls / mut: a mutated Oracle subclass and its attributes (the CPU self-check)."""
    if cls is Oracle:
        return _oracle_scan_cached(c, dtype, tuple(grads))
    return _oracle_scan(c, dtype, tuple(grads), cls, mut)


@functools.lru_cache(maxsize=None)
def _oracle_scan_cached(c, dtype, grads):
    return _oracle_scan(c, dtype, grads, Oracle, {})


def _oracle_scan(c, dtype, grads, cls, mut):
    embed, action, reset, init, ups = scan_inputs(c)
    with oracle_dtype(dtype):
        orc, P = _oracle(c, dtype, cls, ("rssm.",))
        for k, v in mut.items():
            setattr(orc, k, v)
        e = embed.to(dtype).requires_grad_(True)
        st, de, lo = orc.observe(e, action.to(dtype), tuple(x.to(dtype) for x in init), reset, noise_seed(c))
        outs = dict(stoch=st, deter=de, logit=lo)
        loss = sum((outs[k] * ups[k].to(dtype)).sum() for k in grads)
        names = list(P)
        gr = torch.autograd.grad(loss, [e] + [P[k] for k in names], allow_unused=True)
    z = lambda g, like: np.zeros(tuple(like.shape)) if g is None else g.detach().numpy().astype(np.float64)  # noqa: E731
    return dict(idx=st.detach().argmax(-1).numpy(), deter=de.detach().numpy().astype(np.float64),
                logit=lo.detach().numpy().astype(np.float64), d_embed=z(gr[0], e),
                grads={k: z(g, P[k]) for k, g in zip(names, gr[1:])})


def run_oracle_imag(c, dtype=torch.float64, cls=Oracle, **mut):
    if cls is Oracle:
        return _oracle_imag_cached(c, dtype)
    return _oracle_imag(c, dtype, cls, mut)


@functools.lru_cache(maxsize=None)
def _oracle_imag_cached(c, dtype):
    return _oracle_imag(c, dtype, Oracle, {})


def _oracle_imag(c, dtype, cls, mut):
    """Oracle.imagine, time-major like Dreamer._imagine_tm: idx (H1, N, S), deter (H1, N, D), actions (H1, N, A), and
    the logits the margins need."""
    stoch, deter = imag_inputs(c)
    with oracle_dtype(dtype):
        orc, _ = _oracle(c, dtype, cls, ("rssm.", "actor."))
        for k, v in mut.items():
            setattr(orc, k, v)
        rec = {}
        feat, act = orc.imagine((stoch.to(dtype), deter.to(dtype)), c.H1, noise_seed(c), IMAG_ROW_OFFSET, rec)
    SK = c.S * c.K
    feat, act = feat.transpose(0, 1), act.transpose(0, 1)
    out = dict(idx=feat[..., :SK].reshape(c.H1, c.N, c.S, c.K).argmax(-1).numpy(),
               deter=feat[..., SK:].numpy().astype(np.float64), actions=act.numpy().astype(np.float64),
               actor_logit=torch.stack(rec["imag_actor_logit"], 1).numpy().astype(np.float64))
    if c.H1 > 1:
        out["prior_logit"] = torch.stack(rec["imag_prior_logit"], 1).numpy().astype(np.float64)
    return out


# --------------------------------------------------------------------------------------------------- product runs
def run_product_scan(ag, c, grads=ALL_GRADS):
    """RSSM.observe forward + backward on the product; gradients returned under the reference's names / layouts."""
    embed, action, reset, init, ups = scan_inputs(c)
    rssm = ag.rssm
    for p in rssm.parameters():
        if p.grad is not None:
            p.grad.zero_()
    e = embed.cuda().requires_grad_(True)
    st, de, lo = rssm.observe(e, action.cuda(), tuple(x.cuda() for x in init), reset.cuda(), seed=noise_seed(c),
                              row_offset=0)
    outs = dict(stoch=st, deter=de, logit=lo)
    loss = sum((outs[k] * ups[k].cuda()).sum() for k in grads)
    loss.backward()
    torch.cuda.synchronize()
    gr = {}
    for n, p in rssm.named_parameters():
        g = torch.zeros_like(p) if p.grad is None else p.grad.detach()
        gr["rssm." + n] = ag.to_ref_layout(p, g).cpu().numpy().astype(np.float64)
    return dict(idx=st.detach().argmax(-1).cpu().numpy(), deter=de.detach().cpu().numpy().astype(np.float64),
                logit=lo.detach().cpu().numpy().astype(np.float64),
                d_embed=e.grad.detach().cpu().numpy().astype(np.float64), grads=gr,
                raw=(st.detach().clone(), de.detach().clone(), lo.detach().clone(), e.grad.detach().clone(),
                     {n: p.grad.detach().clone() for n, p in rssm.named_parameters() if p.grad is not None}))


def run_product_imag(ag, c):
    stoch, deter = imag_inputs(c)
    f, a = ag._imagine_tm((stoch.cuda(), deter.cuda()), c.H1, seed=noise_seed(c), row_offset=IMAG_ROW_OFFSET)
    torch.cuda.synchronize()
    SK = c.S * c.K
    return dict(idx=f[..., :SK].reshape(c.H1, c.N, c.S, c.K).argmax(-1).cpu().numpy(),
                deter=f[..., SK:].cpu().numpy().astype(np.float64), actions=a.cpu().numpy().astype(np.float64),
                raw=(f.clone(), a.clone()))


# --------------------------------------------------------------------------------------------------- margins
def scan_min_margin(c, ref32):
    """smallest top-2 margin of the Gumbel-perturbed unimix posterior logits (float32 oracle's logits)"""
    spec, _ = spec_params(c)
    return float(post_margins(ref32["logit"], noise_seed(c), spec.unimix).min())


def imag_min_margin(c, ref32):
    """smallest margin over the prior samples and, for a one-hot actor with a choice (A > 1), the action samples"""
    spec, _ = spec_params(c)
    m = np.inf
    if c.H1 > 1:
        m = float(imag_margins(ref32["prior_logit"], noise_seed(c), spec.unimix, IMAG_ROW_OFFSET).min())
    if c.discrete and c.A > 1:
        um = float(spec.actor_dist.unimix_ratio)
        for t in range(c.H1):
            g = nz.gumbel_block(noise_seed(c), nz.STREAM_ACT, t, c.N, IMAG_ROW_OFFSET, c.A)
            m = min(m, float(perturbed_margin(ref32["actor_logit"][:, t], g, um).min()))
    return m


# --------------------------------------------------------------------------------------------------- comparisons
def _ratio(got, ref, rtol, atol):
    """max |got - ref| / (atol + rtol |ref|): the fraction of the bound used; inf for a NaN"""
    r = np.abs(got - ref) / (atol + rtol * np.abs(ref))
    return float(np.nan_to_num(r, nan=np.inf).max()) if r.size else 0.0


def _rel_max(got, ref):
    """(max |got - ref|, max |ref|); the error is inf for a NaN"""
    e = np.abs(got - ref)
    return (float(np.nan_to_num(e, nan=np.inf).max()) if e.size else 0.0), float(np.abs(ref).max()) if e.size else 0.0


def scan_errors(got, ref):
    """The figures compare_scan judges (and DESIGN.md's table records): index mismatches, the worst fraction of the
    state bound used and the worst absolute state error, the gradients' errors relative to each tensor's max."""
    assert got["idx"].shape == ref["idx"].shape
    out = dict(idx_mismatch=int((got["idx"] != ref["idx"]).sum()))
    out["state_ratio"] = max(_ratio(got[k], ref[k], STATE_RTOL, STATE_ATOL) for k in ("deter", "logit"))
    out["state_abs"] = max(_rel_max(got[k], ref[k])[0] for k in ("deter", "logit"))
    e, s = _rel_max(got["d_embed"], ref["d_embed"])
    out["embed"] = (e, s)
    assert set(got["grads"]) == set(ref["grads"]), set(got["grads"]) ^ set(ref["grads"])
    out["params"] = {k: _rel_max(got["grads"][k], ref["grads"][k]) for k in ref["grads"]}
    return out


def scan_summary(err):
    """one line of figures: states, embed gradient and the worst parameter gradient relative to its tensor's max"""
    rel = lambda es: es[0] / es[1] if es[1] > 0 else es[0]  # noqa: E731
    worst = max(err["params"], key=lambda k: rel(err["params"][k]))
    return dict(idx_mismatch=err["idx_mismatch"], state_abs=err["state_abs"], state_ratio=err["state_ratio"],
                embed_rel=rel(err["embed"]), param_rel=rel(err["params"][worst]), param=worst)


def compare_scan(got, ref, what=""):
    err = scan_errors(got, ref)
    bad = []
    if err["idx_mismatch"]:
        bad.append(f"{err['idx_mismatch']} posterior indices differ")
    if not err["state_ratio"] <= 1.0:
        bad.append(f"deter / logit use {err['state_ratio']:.3g} of the {STATE_ATOL} + {STATE_RTOL} |ref| bound")
    for k, (e, s) in [("d_embed", err["embed"])] + sorted(err["params"].items()):
        if not e <= GRAD_REL * s + GRAD_ABS:
            bad.append(f"grad {k}: error {e:.3g}, tensor max {s:.3g}")
    assert not bad, f"{what}: " + "; ".join(bad)
    return err


def imag_errors(got, ref, discrete):
    assert got["idx"].shape == ref["idx"].shape and got["actions"].shape == ref["actions"].shape
    out = dict(idx_mismatch=int((got["idx"] != ref["idx"]).sum()), act_mismatch=0)
    if discrete:
        out["act_mismatch"] = int((got["actions"].argmax(-1) != ref["actions"].argmax(-1)).sum())
    for k in ("deter", "actions"):
        out[k + "_ratio"] = _ratio(got[k], ref[k], IMAG_RTOL, IMAG_ATOL)
        out[k + "_abs"] = _rel_max(got[k], ref[k])[0]
    return out


def compare_imag(got, ref, discrete, what=""):
    err = imag_errors(got, ref, discrete)
    bad = []
    if err["idx_mismatch"]:
        bad.append(f"{err['idx_mismatch']} imagined indices differ")
    if err["act_mismatch"]:
        bad.append(f"{err['act_mismatch']} one-hot actions differ")
    for k in ("deter", "actions"):
        if not err[k + "_ratio"] <= 1.0:
            bad.append(f"{k} uses {err[k + '_ratio']:.3g} of the {IMAG_ATOL} + {IMAG_RTOL} |ref| bound")
    assert not bad, f"{what}: " + "; ".join(bad)
    return err


# --------------------------------------------------------------------------------------------------- the C gate
def imagine_work_status(D, G, S, K, A=6, discrete=False, actor_layers=3, img_layers=2, N=64, H1=3):
    """sd_imagine_work_floats on a descriptor of these shapes and no pointers: the float count, or a negative status
    (nat.SD_ESHAPE for a shape outside csrc/img.hip's gate). Launches nothing and touches no device."""
    from sdreamer import _native as nat
    d = nat.ImagineDesc()
    d.N, d.H1, d.D, d.U, d.SK, d.Kd, d.G, d.A = N, H1, D, 256, S * K, K, G, A
    d.act_discrete, d.actor_layers, d.img_layers = int(discrete), actor_layers, img_layers
    return nat.fns["sd_imagine_work_floats"](ctypes.addressof(d))
