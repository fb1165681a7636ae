"""Cases, inputs, float64 references and comparisons for the small row kernels between the fused pieces:
csrc/rownorm.hip (RMSNorm + SiLU, column sums), csrc/dist.hip (sampler, KL, two-hot, replay-value and actor-critic
losses, bounded normal, Bernoulli, GRU gates) and csrc/returns.hip (λ-return, ReturnEMA). Test infrastructure (a plain
module: no fixtures, no pytest hooks), in the pattern of small_models.py / conv_models.py.

Shared by tests/test_rowop_parity_cpu.py (the tables reach every dispatch arm, the input conditions hold, the float32
restatement passes every comparison with room, planted faults fail it) and tests/test_gpu_rowops_f64.py (the kernels
against float64). DESIGN.md § 2.3 holds the tables and the measured figures.

A reference is one function `ref_<family>(case, dt, fault)`: the oracle's own functions (oracle/ref_cpu.py, its
arithmetic type switched by small_models.oracle_dtype) or, where the oracle has none, a torch restatement of the
reference's expression, evaluated in `dt` with torch autograd. dt = float64 is the reference, dt = float32 the
restatement whose distance from float64 sizes the tolerances, `fault` plants one named error. It returns
{output: ndarray}; an output that is a sum also returns `output@scale`, the Σ|terms| of each element.

Comparison (compare / ratios): every output elementwise through parity.assert_close with rtol = 0 and
  atol_i = tol * max(|ref_i|, 1)       for a pointwise output,
  atol_i = k * eps32 * scale_i         for a sum (scale_i = the float64 Σ|terms| of that element),
and, for both, the existing tests' figure in the existing tests' form as a cap: max|err| <= cap * max(max|ref|, 1)
(test_gpu_ops.py close()). Indices and the quantiles are compared exactly.
"""
import functools
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

import parity
import small_models as sm
from oracle import noise as nz
from oracle import ref_cpu as R

F32, F64 = torch.float32, torch.float64
EPS32 = float(np.finfo(np.float32).eps)
RMS_EPS = 1e-4  # kernels.EPS: nn.RMSNorm(eps=1e-04)
MIN_MARGIN = sm.MIN_MARGIN
UNIMIX = 0.01
DISC, LAMB = 1 - 1 / 333, 0.95


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _np(t):
    return t.detach().cpu().numpy()


# =============================================================================================== arm functions
def team_for(N):
    """rownorm.hip:352-356 team_for"""
    return 16 if N <= 64 else 64 if N <= 1024 else 256


def pick_vpt(n):
    """rownorm.hip:314-321 pick_vpt"""
    return n if n <= 4 else 8 if n <= 8 else 16


def rms_arm(N, aligned=True, ldy=None, ldx=None):
    """rownorm.hip:347-350 vec_ok + 371-383 / 415-424: ("vec", NV) or (team, VPT). The forward passes its ldy alone;
    the backward needs both leading dimensions and every pointer (x, w, dx, dy) 16-B aligned."""
    ldy = N if ldy is None else ldy
    ldx = N if ldx is None else ldx
    if aligned and N in (256, 512, 1024) and ldy % 4 == 0 and ldx % 4 == 0:
        return ("vec", N // 256)
    t = team_for(N)
    return (t, pick_vpt((N + t - 1) // t))


def rms_padded_width(arm):
    return 256 * arm[1] if arm[0] == "vec" else arm[0] * arm[1]


def rms_rows_per_block(N):
    """teams per 256-thread block (rownorm.hip:27, 62; the vector forms: a wave per row, :135, :170)"""
    return 256 // team_for(N)


def rms_fwd_blocks(M, N):
    """rownorm.hip:323-328 grid_for"""
    return min(-(-M // rms_rows_per_block(N)), 8192)


def rms_bwd_blocks(M, N):
    """rownorm.hip:330-334 grid_bwd, 388-391 sd_rmsnorm_bwd_blocks"""
    return min(rms_fwd_blocks(M, N), 512)


COLSUM_RCH = 512  # rownorm.hip:223


def colsum_chunks(R_):
    """rownorm.hip:430 sd_colsum_chunks"""
    return -(-R_ // COLSUM_RCH)


def colsum_arm(R_, N, has_ws):
    """rownorm.hip:437-452 sd_colsum_ws"""
    ch = colsum_chunks(R_)
    if ch <= 1 and N <= 4096:
        return "short"
    if ch <= 1 or not has_ws:
        return "kernel"
    return "two_pass"


def team(K):
    """dist.hip:605 team_pow2"""
    return 8 if K <= 8 else 16 if K <= 16 else 32 if K <= 32 else 64


def lret_arm(T, term, cont):
    """returns.hip:277-282 sd_lambda_return_strided"""
    return "staged" if T <= 255 and not (term and cont) else "unstaged"


def ema_arm(n):
    """returns.hip:175, 193 RE_KPT / in_regs"""
    return "regs" if n <= 16384 else "global"


RMS_ARMS_UNREACHABLE = {
    (64, 1): "team 64 serves N >= 65, so ceil(N / 64) >= 2",
    (256, 1): "team 256 serves N >= 1025, so ceil(N / 256) >= 5 -> VPT 8 or 16",
    (256, 2): "as (256, 1)", (256, 3): "as (256, 1)", (256, 4): "as (256, 1)",
    (16, 8): "team 16 serves N <= 64, so ceil(N / 16) <= 4", (16, 16): "as (16, 8)",
}
RMS_ARMS_REACHABLE = ([(t, v) for t in (16, 64, 256) for v in (1, 2, 3, 4, 8, 16) if (t, v) not in RMS_ARMS_UNREACHABLE]
                      + [("vec", 1), ("vec", 2), ("vec", 4)])


# =============================================================================================== tolerances
@dataclass(frozen=True)
class Tol:
    cap: float  # the existing tests' figure (max error over max(max|ref|, 1)); never loosened
    tol: float  # pointwise: of max(|ref_i|, 1); sum: multiple of eps32 * scale_i
    kind: str = "pt"  # "pt" | "sum" | "exact"

    @property
    def capped(self):
        return self.kind == "pt" and self.tol >= self.cap


EXACT = Tol(0.0, 0.0, "exact")
# Each tolerance is 8 x the larger of two measured distances from float64, in the output's own unit (units()): the
# float32 restatement's on the CPU and the kernel's on the MI355X (DESIGN.md § 2.3 lists all three per output). Where
# that exceeds the cap, the cap is the tolerance (Tol.capped): 1e-6 is 8.4 float32 epsilons, so on O(1) values two
# correct float32 evaluations already use a quarter of it.
TOL = {
    "rms": {"y": Tol(2e-6, 2e-6), "rstd": Tol(2e-6, 1.3e-6), "dx": Tol(1e-5, 4e-6), "dw": Tol(1e-5, 20.0, "sum")},
    "colsum": {"out": Tol(1e-5, 4.0, "sum")},
    # value: (hard - ys) + ys rounds once (both measured 0): 2 float32 epsilons
    "sample": {"value": Tol(1e-6, 2 * EPS32), "index": EXACT, "entropy": Tol(1e-5, 2.5e-6),
               "dlogits": Tol(2e-5, 1.5e-6), "dlogits_acc": Tol(2e-5, 1.5e-6)},
    "logp": {"logp": Tol(1e-5, 1.6e-6), "ent": Tol(1e-5, 2.5e-6), "dl_both": Tol(1e-5, 3e-6), "dl_lp": Tol(1e-5, 3e-6),
             "dl_ent": Tol(1e-5, 2e-6)},
    "kl": {"kl": Tol(1e-5, 14.0, "sum"), "dyn": Tol(1e-5, 14.0, "sum"), "rep": Tol(1e-5, 14.0, "sum"),
           "d_post": Tol(1e-5, 1e-5), "d_prior": Tol(1e-5, 3e-6), "d_post_acc": Tol(1e-5, 1e-5),
           "d_prior_acc": Tol(1e-5, 3e-6)},
    "twohot": {"mode": Tol(1e-5, 8.0, "sum"), "dmode": Tol(1e-5, 8.0, "sum"), "logp": Tol(1e-5, 2e-6),
               "dlogits": Tol(1e-5, 1.5e-6), "dlogits_acc": Tol(1e-5, 1.5e-6)},
    "repval": {"rows": Tol(1e-5, 1e-6), "loss": Tol(1e-5, 8.0, "sum"), "dlogits": Tol(1e-5, 2.5e-7)},
    "imag_ac": {"rows_v": Tol(1e-5, 1.5e-6), "rows_p": Tol(1e-5, 1e-6), "adv": Tol(1e-6, 7.5e-7),
                "policy": Tol(1e-5, 4.0, "sum"), "value": Tol(1e-5, 4.0, "sum"), "dvl": Tol(1e-6, 1e-7),
                "dlogpi": Tol(1e-6, 8.5e-7), "dent": Tol(1e-6, 4e-11)},
    "bnormal": {"logp": Tol(1e-5, 18.0, "sum"), "ent": Tol(1e-5, 12.0, "sum"), "dx_both": Tol(1e-5, 22.0, "sum"),
                "dx_lp": Tol(1e-5, 23.0, "sum"), "dx_ent": Tol(1e-5, 14.0, "sum")},
    "bernoulli": {"logp": Tol(1e-6, 1e-6), "mean": Tol(1e-6, 6e-7), "dlogit": Tol(1e-6, 1e-6)},
    "gru": {"out": Tol(1e-6, 1e-6), "dgates": Tol(1e-6, 1e-6), "dh": Tol(1e-6, 1e-6), "dh_acc": Tol(1e-6, 1e-6)},
    "lret": {"ret": Tol(1e-5, 8.5e-6), "cont": Tol(1e-6, 8e-7), "weight": Tol(1e-6, 9.5e-7)},
    # the existing 1e-7 is a distance between two float32 evaluations; against float64 the two roundings of each EMA
    # step are the floor, so the EMA is a sum of its two terms here, inside the tightest cap of the other heads
    "ema": {"q1": EXACT, "q2": EXACT, "ema1": Tol(1e-6, 13.0, "sum"), "os1": Tol(1e-6, 13.0, "sum"),
            "ema2": Tol(1e-6, 13.0, "sum"), "os2": Tol(1e-6, 13.0, "sum")},
}
for _fam in TOL.values():
    assert all(t.kind != "pt" or t.tol <= t.cap for t in _fam.values())


def outputs(ref):
    return [k for k in ref if "@" not in k]


def _atol(t, ref, name):
    r = np.asarray(ref[name], np.float64)
    if t.kind == "sum":
        return t.tol * EPS32 * np.asarray(ref[name + "@scale"], np.float64)
    return t.tol * np.maximum(np.abs(r), 1.0)


def _cap_ratio(t, got, r):
    if r.size == 0:
        return 0.0
    return float(np.abs(got - r).max() / (t.cap * max(np.abs(r).max(), 1.0)))


def ratios(fam, got, ref):
    """{output: (fraction of the elementwise bound used, fraction of the cap used)}; exact outputs: 0 or inf"""
    out = {}
    for name in outputs(ref):
        if name not in got:
            continue
        t = TOL[fam][name]
        g, r = np.asarray(got[name]), np.asarray(ref[name])
        assert g.shape == r.shape, (fam, name, g.shape, r.shape)
        if t.kind == "exact":
            out[name] = (0.0 if np.array_equal(g, r) else float("inf"),) * 2
        else:
            g, r = g.astype(np.float64), r.astype(np.float64)
            out[name] = (parity.bound_ratio(g, r, 0.0, _atol(t, ref, name)), _cap_ratio(t, g, r))
    return out


def units(fam, got, ref):
    """{output: max error in the output's own unit}: max(|ref_i|, 1) (pointwise) or eps32 * scale_i (sum) — the figure
    a tolerance is chosen from (times 8, inside the cap)"""
    out = {}
    for name in outputs(ref):
        t = TOL[fam][name]
        if name not in got or t.kind == "exact" or np.asarray(ref[name]).size == 0:
            continue
        one = Tol(t.cap, 1.0, t.kind)
        out[name] = parity.bound_ratio(np.asarray(got[name], np.float64), np.asarray(ref[name], np.float64), 0.0,
                                       _atol(one, ref, name))
    return out


def summary(rt):
    return " ".join(f"{k}={a:.2g}/{b:.2g}" for k, (a, b) in rt.items())


def compare(fam, got, ref, what=""):
    for name in outputs(ref):
        if name not in got:
            continue
        t = TOL[fam][name]
        g, r = np.asarray(got[name]), np.asarray(ref[name])
        assert g.shape == r.shape, (what, name, g.shape, r.shape)
        if t.kind == "exact":
            assert np.array_equal(g, r), f"{what} {name}: {int((g != r).sum())} of {r.size} differ"
            continue
        if r.size == 0:
            continue
        g, r = g.astype(np.float64), r.astype(np.float64)
        assert np.isfinite(g).all(), f"{what} {name}: not finite"
        parity.assert_close(g, r, 0.0, _atol(t, ref, name), f"{what} {name}")
        assert _cap_ratio(t, g, r) <= 1.0, f"{what} {name}: above the cap {t.cap} of max(max|ref|, 1)"


def passes(fam, got, ref):
    return all(a <= 1.0 and b <= 1.0 for a, b in ratios(fam, got, ref).values())


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in outputs(a))


# =============================================================================================== RMSNorm + SiLU
@dataclass(frozen=True)
class RmsCase:
    M: int
    N: int
    layout: str = "plain"  # plain | ld4 | ld1 | mis | dymis
    bwd: bool = True
    acc_dx: bool = False
    dw: object = "acc"  # "acc" (onto a prefilled dw) | "set" (accumulate_dw = False) | None
    eps: object = None
    zero_row: bool = False

    @property
    def name(self):
        s = f"{self.M}x{self.N}"
        for flag, tag in ((self.layout != "plain", self.layout), (not self.bwd, "fwd"), (self.acc_dx, "accdx"),
                          (self.dw != "acc", f"dw{self.dw}"), (self.eps is not None, "eps"), (self.zero_row, "zrow")):
            if flag:
                s += "-" + tag
        return s

    def blocks(self):
        """(width, first column) of the buffers y / dx / dy live in"""
        N = self.N
        wide = {"ld4": (N + 4, 4), "ld1": (N + 1, 0), "mis": (N + 4, 1)}.get(self.layout, (N, 0))
        return {"y": wide, "dx": wide, "dy": (N + 4, 1) if self.layout == "dymis" else (N, 0)}

    def arms(self):
        b = self.blocks()
        al = lambda k: b[k][1] % 4 == 0  # noqa: E731  (the buffers themselves start 16-B aligned)
        fwd = rms_arm(self.N, al("y"), b["y"][0])
        bwd = rms_arm(self.N, al("dx") and al("dy"), b["dy"][0], b["dx"][0]) if self.bwd else None
        return fwd, bwd


RMS_CASES = (
    [RmsCase(*mn) for mn in ((3, 1), (5, 16), (5, 17), (7, 49), (7, 64),  # team 16, VPT 1, 1, 2, 4, 4
                             (7, 33),  # team 16, VPT 3
                             (5, 65), (5, 129), (5, 193), (5, 257), (3, 513), (3, 1000),  # team 64
                             (3, 1025), (3, 2049), (2, 4096),  # team 256
                             (5, 256), (5, 512), (5, 1024))]  # vector
    + [RmsCase(5, 256, layout=l) for l in ("ld4", "ld1", "mis", "dymis")]
    + [RmsCase(*mn) for mn in ((8195, 16), (2051, 65), (515, 1025), (2051, 256))]  # grid-stride backward
    + [RmsCase(*mn, bwd=False) for mn in ((131075, 8), (32771, 65), (8195, 1025), (32771, 256))]
    + [RmsCase(5, n, **kw) for n in (65, 256)
       for kw in (dict(acc_dx=True), dict(dw="set"), dict(dw=None), dict(eps=EPS32), dict(zero_row=True))])
RMS = {c.name: c for c in RMS_CASES}
assert len(RMS) == len(RMS_CASES)


@functools.lru_cache(maxsize=None)
def rms_inputs(c):
    g = _g(1000 * c.M + c.N)
    x = torch.randn(c.M, c.N, generator=g) * 2
    if c.zero_row:
        x[c.M // 2] = 0.0
    w = 1 + 0.1 * torch.randn(c.N, generator=g)
    d = {"x": x, "w": w}
    if c.bwd:
        d.update(dy=torch.randn(c.M, c.N, generator=g), dx0=torch.randn(c.M, c.N, generator=g),
                 dw0=torch.randn(c.N, generator=g))
    return d


def ref_rms(c, act, dt=F64, fault=None):
    """F.rms_norm (oracle ref_cpu.rms, ref_cpu.py:155-156: nn.RMSNorm(eps)) then F.silu, and its autograd gradient.
    faults: "rms_padded_mean" the mean of x^2 over the arm's team-padded width; "dw_first_stride" dw from the rows of
    the first grid stride only; "acc_dx_ignored"."""
    i = rms_inputs(c)
    eps = RMS_EPS if c.eps is None else c.eps
    x, w = i["x"].to(dt).requires_grad_(), i["w"].to(dt).requires_grad_()
    fwd_arm, bwd_arm = c.arms()
    pad = rms_padded_width(fwd_arm) - c.N if fault == "rms_padded_mean" else 0

    def fwd(xx, ww):
        if pad:  # zero columns widen the mean's divisor and nothing else
            return F.rms_norm(F.pad(xx, (0, pad)), (c.N + pad,), F.pad(ww, (0, pad)), eps)[:, :c.N]
        return F.rms_norm(xx, (c.N,), ww, eps)

    z = fwd(x, w)
    y = F.silu(z) if act else z
    out = {"y": _np(y), "rstd": _np((x.detach().pow(2).sum(-1) / (c.N + pad) + eps).rsqrt())}
    if not c.bwd:
        return out
    dy = i["dy"].to(dt)
    first = rms_bwd_blocks(c.M, c.N) * rms_rows_per_block(c.N) if fault == "dw_first_stride" else c.M
    dx, dw_all = torch.autograd.grad(y, (x, w), dy, retain_graph=first < c.M)
    if first < c.M:
        dym = dy.clone()
        dym[first:] = 0
        dw_all = torch.autograd.grad(y, w, dym)[0]
    if c.acc_dx and fault != "acc_dx_ignored":
        dx = dx + i["dx0"].to(dt)
    out["dx"] = _np(dx)
    if c.dw is not None:
        xhat = x.detach() * torch.as_tensor(out["rstd"])[:, None]
        scale = (dy * xhat).abs().sum(0)
        if c.dw == "acc":
            dw_all, scale = dw_all + i["dw0"].to(dt), scale + i["dw0"].to(dt).abs()
        out["dw"], out["dw@scale"] = _np(dw_all), _np(scale)
    return out


# =============================================================================================== column sums
@dataclass(frozen=True)
class ColsumCase:
    R: int
    N: int
    ld: object = None
    ws: bool = True  # K.colsum hands a workspace over when R > 512; False: sd_colsum (none)
    accumulate: bool = True

    @property
    def name(self):
        return (f"{self.R}x{self.N}" + (f"-ld{self.ld}" if self.ld else "") + ("" if self.ws else "-nows")
                + ("" if self.accumulate else "-set"))

    def arm(self):
        return colsum_arm(self.R, self.N, self.ws)


COLSUM_CASES = ([ColsumCase(*rn) for rn in ((1, 1), (31, 33), (33, 31), (127, 65), (129, 64), (512, 4096),
                                             (512, 4097), (513, 33))]
                + [ColsumCase(513, 33, ws=False), ColsumCase(1029, 255, ld=300),
                   ColsumCase(127, 65, accumulate=False), ColsumCase(513, 33, accumulate=False),
                   ColsumCase(512, 4097, accumulate=False)])
COLSUM = {c.name: c for c in COLSUM_CASES}
assert len(COLSUM) == len(COLSUM_CASES)
COLSUM_STEP = {"short": 128, "kernel": 32, "two_pass": COLSUM_RCH}  # rows per unrolled step / per chunk


@functools.lru_cache(maxsize=None)
def colsum_inputs(c):
    g = _g(7 * c.R + c.N)
    buf = torch.randn(c.R, c.ld or c.N, generator=g)
    return {"buf": buf, "col0": (c.ld - c.N) // 2 if c.ld else 0, "out0": torch.randn(c.N, generator=g)}


def ref_colsum(c, dt=F64, fault=None):
    """x.sum(0) (+ out). fault "colsum_drop_tail": without the rows after the last whole unrolled step / chunk."""
    i = colsum_inputs(c)
    x = i["buf"][:, i["col0"]:i["col0"] + c.N].to(dt)
    if fault == "colsum_drop_tail":
        step = COLSUM_STEP[c.arm()]
        if c.R % step:
            x = x[:c.R - c.R % step]
    s, scale = x.sum(0), x.abs().sum(0)
    if c.accumulate:
        s, scale = s + i["out0"].to(dt), scale + i["out0"].to(dt).abs()
    return {"out": _np(s), "out@scale": _np(scale) + 1e-30}


# =============================================================================================== teamed heads
TEAM_KS = (1, 2, 6, 8, 9, 16, 17, 32, 33, 63, 64)
SAMPLE_STEP, SAMPLE_OFFSET = 7, 5


def team_groups(K):
    """one group, and a count that leaves the last 256-thread block partly filled"""
    return (1, 2 * (256 // team(K)) + 3)


@dataclass(frozen=True)
class TeamCase:
    K: int
    groups: int

    @property
    def name(self):
        return f"K{self.K}-g{self.groups}"

    @property
    def seed(self):
        return 4242 + 131 * self.K + self.groups


TEAM_CASES = [TeamCase(K, n) for K in TEAM_KS for n in team_groups(K)]
TEAMC = {c.name: c for c in TEAM_CASES}


@functools.lru_cache(maxsize=None)
def sample_inputs(c):
    g = _g(c.seed)
    n, K = c.groups, c.K
    gum = nz.gumbel(c.seed, nz.STREAM_IMG, SAMPLE_STEP, np.arange(n * K, dtype=np.int64) + SAMPLE_OFFSET * K)
    return {"logits": torch.randn(n, K, generator=g) * 3, "gumbel": torch.from_numpy(gum).view(n, K),
            "dout": torch.randn(n, K, generator=g), "dl0": torch.randn(n, K, generator=g),
            "action": F.one_hot(torch.randint(0, K, (n,), generator=g), K).float(),
            "glogp": torch.randn(n, generator=g), "gent": torch.randn(n, generator=g)}


def _norm_logits(l, dt, fault):
    if fault == "unimix_omitted":
        return torch.log_softmax(l, -1)
    with sm.oracle_dtype(dt):
        return R.unimix_logits(l, UNIMIX)


def ref_sample(c, dt=F64, fault=None):
    """OneHotDist + rsample (oracle unimix_logits / st_gumbel_sample / cat_entropy); fault "unimix_omitted"."""
    i = sample_inputs(c)
    l = i["logits"].to(dt).requires_grad_()
    nl = _norm_logits(l, dt, fault)
    g = i["gumbel"].to(dt)
    st = R.st_gumbel_sample(nl, g)
    dl = torch.autograd.grad(st, l, i["dout"].to(dt))[0]
    pert = (nl + g).detach()
    top = torch.topk(pert, min(2, c.K), -1).values
    margin = (top[:, 0] - top[:, 1]).min().item() if c.K > 1 else float("inf")
    return {"value": _np(st), "index": _np(pert.argmax(-1)).astype(np.int32), "entropy": _np(R.cat_entropy(nl)),
            "dlogits": _np(dl), "dlogits_acc": _np(dl + i["dl0"].to(dt)), "@margin": margin}


def ref_logp(c, dt=F64, fault=None):
    """discrete actor: OneHotCategorical.log_prob / entropy on the unimix logits (oracle onehot_log_prob, cat_entropy)"""
    i = sample_inputs(c)
    l = i["logits"].to(dt).requires_grad_()
    nl = _norm_logits(l, dt, fault)
    lp, ent = R.onehot_log_prob(nl, i["action"].to(dt)), R.cat_entropy(nl)
    g1, g2 = i["glogp"].to(dt), i["gent"].to(dt)
    d_lp = torch.autograd.grad(lp, l, g1, retain_graph=True)[0]
    d_ent = torch.autograd.grad(ent, l, g2)[0]
    return {"logp": _np(lp), "ent": _np(ent), "dl_both": _np(d_lp + d_ent), "dl_lp": _np(d_lp), "dl_ent": _np(d_ent)}


# ----------------------------------------------------------------------------------------------- KL
@dataclass(frozen=True)
class KlCase:
    S: int
    K: int
    rows: int = 5

    @property
    def name(self):
        return f"S{self.S}-K{self.K}-r{self.rows}"


KL_CASES = [KlCase(1, 1), KlCase(3, 6), KlCase(33, 8), KlCase(5, 17), KlCase(5, 33), KlCase(8, 64), KlCase(64, 16),
            KlCase(3, 6, 4099)]
KL = {c.name: c for c in KL_CASES}
KL_FREE_GAP = 1e-3


@functools.lru_cache(maxsize=None)
def kl_inputs(c):
    g = _g(100 * c.S + c.K + c.rows)
    sh = (c.rows, c.S * c.K)
    d = {"post": torch.randn(sh, generator=g) * 3, "prior": torch.randn(sh, generator=g) * 3,
         "g_rep": torch.randn(c.rows, generator=g), "g_dyn": torch.randn(c.rows, generator=g),
         "dpost0": torch.randn(sh, generator=g), "dprior0": torch.randn(sh, generator=g)}
    kl = np.sort(_np(R.kl_cat(d["post"].double().view(c.rows, c.S, c.K),
                              d["prior"].double().view(c.rows, c.S, c.K)).sum(-1)))
    # free nats: the middle of the widest gap between neighbouring rows' float64 KL (rows on both sides, none near);
    # K = 1 has KL = 0 in every row: free = 1 puts every row below
    gaps = np.diff(kl)
    j = int(np.argmax(gaps)) if len(gaps) and gaps.max() > 0 else None
    d["free"] = float(np.float32((kl[j] + kl[j + 1]) / 2)) if j is not None else 1.0
    return d


def ref_kl(c, dt=F64, fault=None):
    """RSSM.kl_loss (oracle kl_cat, ref_cpu.py:80-84; rssm.py:222-230: clip(sum_S KL, min=free), sg on one side each).
    faults: "kl_grad_below_free", "kl_s_minus_1"."""
    i = kl_inputs(c)
    sh = (c.rows, c.S, c.K)
    p, q = i["post"].to(dt).requires_grad_(), i["prior"].to(dt).requires_grad_()
    S_ = c.S - 1 if fault == "kl_s_minus_1" else c.S
    pv, qv = p.view(sh)[:, :S_], q.view(sh)[:, :S_]
    rep_raw, dyn_raw = R.kl_cat(pv, qv.detach()).sum(-1), R.kl_cat(pv.detach(), qv).sum(-1)
    clip = (lambda t: t) if fault == "kl_grad_below_free" else (lambda t: torch.clip(t, min=i["free"]))
    (i["g_rep"].to(dt) * clip(rep_raw) + i["g_dyn"].to(dt) * clip(dyn_raw)).sum().backward()
    dp = p.grad if p.grad is not None else torch.zeros_like(p)
    dq = q.grad if q.grad is not None else torch.zeros_like(q)
    lpa, lpb = torch.log_softmax(pv.detach(), -1), torch.log_softmax(qv.detach(), -1)
    scale = (lpa.exp() * (lpa.abs() + lpb.abs())).sum((-1, -2)) + 1e-30
    kl = rep_raw.detach()
    cl = torch.clip(kl, min=i["free"])
    return {"kl": _np(kl), "dyn": _np(cl), "rep": _np(cl), "kl@scale": _np(scale), "dyn@scale": _np(scale) + i["free"],
            "rep@scale": _np(scale) + i["free"], "d_post": _np(dp), "d_prior": _np(dq),
            "d_post_acc": _np(dp + i["dpost0"].to(dt)), "d_prior_acc": _np(dq + i["dprior0"].to(dt))}


# =============================================================================================== two-hot family
@dataclass(frozen=True)
class TwohotCase:
    NB: int
    rows: int

    @property
    def name(self):
        return f"NB{self.NB}-r{self.rows}"


TWOHOT_NBS = (1, 3, 63, 65, 129, 255, 256)
TWOHOT_CASES = [TwohotCase(nb, r) for nb in TWOHOT_NBS for r in (1, 5, 65)]
TWOHOT = {c.name: c for c in TWOHOT_CASES}
TARGET_KINDS = ("between", "on_bin", "below_first", "above_last", "zero")  # row r takes kind r % 5 (rows < 5 * 2)


def bins_f32(NB):
    with sm.oracle_dtype(F32):
        return R.twohot_bins(NB)


def _targets(bins, rows, g):
    NB = len(bins)
    i = NB // 3
    j = min(i + 1, NB - 1)
    kinds = {"on_bin": bins[i].item(), "between": (0.3 * bins[i] + 0.7 * bins[j]).item(), "below_first": -1e9,
             "above_last": 1e9, "zero": 0.0}
    t = torch.randn(rows, generator=g) * 30
    for r in range(min(rows, 10)):
        t[r] = kinds[TARGET_KINDS[r % 5]]
    return t


def _peaked_logits(rows, NB, g):
    return -0.5 * (torch.arange(NB) - (NB - 1) // 2).abs().float() + torch.randn(rows, NB, generator=g)


@functools.lru_cache(maxsize=None)
def twohot_inputs(c):
    g = _g(10 * c.NB + c.rows)
    bins = bins_f32(c.NB)
    return {"bins": bins, "logits": _peaked_logits(c.rows, c.NB, g), "target": _targets(bins, c.rows, g),
            "g": torch.randn(c.rows, generator=g), "dl0": torch.randn(c.rows, c.NB, generator=g)}


def twohot_logp(logits, bins, target, fault=None):
    """TwoHot.log_prob: the oracle's (ref_cpu.py:109-128, distributions.py:100-129); fault "twohot_swapped" restates it
    with the two weights exchanged."""
    if fault != "twohot_swapped":
        return R.twohot_log_prob(logits, bins, target.unsqueeze(-1))
    nb = len(bins)
    below = torch.clamp((bins <= target.unsqueeze(-1)).to(torch.int32).sum(-1) - 1, 0, nb - 1)
    above = torch.clamp(nb - (bins > target.unsqueeze(-1)).to(torch.int32).sum(-1), 0, nb - 1)
    equal = below == above
    one = torch.tensor(1.0, dtype=logits.dtype)
    d_below = torch.where(equal, one, (bins[below] - target).abs())
    d_above = torch.where(equal, one, (bins[above] - target).abs())
    total = d_below + d_above
    w_below, w_above = d_below / total, d_above / total  # exchanged
    dist = (F.one_hot(below, nb).to(logits.dtype) * w_below.unsqueeze(-1)
            + F.one_hot(above, nb).to(logits.dtype) * w_above.unsqueeze(-1))
    return (dist * (logits - torch.logsumexp(logits, dim=-1, keepdim=True))).sum(-1)


def ref_twohot(c, dt=F64, fault=None):
    """TwoHot.mode (oracle twohot_mode, odd NB) and log_prob, with their autograd gradients"""
    i = twohot_inputs(c)
    bins, t = i["bins"].to(dt), i["target"].to(dt)
    out = {}
    with sm.oracle_dtype(dt):
        l = i["logits"].to(dt).requires_grad_()
        lp = twohot_logp(l, bins, t, fault)
        dl = torch.autograd.grad(lp, l, i["g"].to(dt))[0]
        out.update(logp=_np(lp), dlogits=_np(dl), dlogits_acc=_np(dl + i["dl0"].to(dt)))
        if c.NB % 2 == 1:
            l = i["logits"].to(dt).requires_grad_()
            mode = R.twohot_mode(l, bins).squeeze(-1)
            dm = torch.autograd.grad(mode, l, i["g"].to(dt))[0]
            # terms p_j b_j; float32 exp(l_j - max) carries (1 + |l_j - max|) roundings of its argument
            ld = l.detach()
            pc = torch.softmax(ld, -1) * (1 + (ld - ld.max(-1, keepdim=True).values).abs())
            ms = (pc * bins.abs()).sum(-1, keepdim=True)
            out.update(mode=_np(mode), dmode=_np(dm))
            out["mode@scale"] = _np(ms.squeeze(-1)) + 1e-30
            out["dmode@scale"] = _np(i["g"].to(dt).abs()[:, None] * pc * (bins.abs() + ms)) + 1e-30
    return out


@dataclass(frozen=True)
class RepvalCase:
    B: int
    Tl: int
    Tr: int
    NB: int = 255

    @property
    def name(self):
        return f"B{self.B}-Tl{self.Tl}-Tr{self.Tr}"


REPVAL_CASES = [RepvalCase(1, 2, 1), RepvalCase(3, 5, 4), RepvalCase(2, 3, 3), RepvalCase(5, 4, 2)]
REPVAL = {c.name: c for c in REPVAL_CASES}
REPVAL_GSCALE = 0.3


@functools.lru_cache(maxsize=None)
def repval_inputs(c):
    g = _g(100 * c.B + 10 * c.Tl + c.Tr)
    bins = bins_f32(c.NB)
    last = (torch.rand(c.B, c.Tl, generator=g) < 0.25).float()
    if c.B > 1:
        last[1, 0], last[0, 0] = 1.0, 0.0
    return {"bins": bins, "logits": _peaked_logits(c.B * c.Tl, c.NB, g).view(c.B, c.Tl, c.NB),
            "ret": _targets(bins, c.B * c.Tr, g).view(c.B, c.Tr),
            "slow": _targets(bins, c.B * c.Tl, g).flip(0).view(c.B, c.Tl), "last": last}


def ref_repval(c, dt=F64, fault=None):
    """dreamer.py:652-658: mean((1 - last) * (-logp(ret) - logp(slow))) over the first Tr of Tl steps (oracle
    twohot_log_prob). fault "repval_row_stride": logits row b * Tr + t instead of b * Tl + t."""
    i = repval_inputs(c)
    bins = i["bins"].to(dt)
    with sm.oracle_dtype(dt):
        l = i["logits"].to(dt).requires_grad_()
        lv = l[:, :c.Tr]
        if fault == "repval_row_stride":
            lv = l.reshape(c.B * c.Tl, c.NB)[:c.B * c.Tr].view(c.B, c.Tr, c.NB)
        w = 1.0 - i["last"].to(dt)[:, :c.Tr]
        rows = w * (-twohot_logp(lv, bins, i["ret"].to(dt)) - twohot_logp(lv, bins, i["slow"].to(dt)[:, :c.Tr]))
        loss = rows.mean()
        dl = torch.autograd.grad(loss * REPVAL_GSCALE, l)[0]
    return {"rows": _np(rows.reshape(-1)), "loss": _np(loss.reshape(1)),
            "loss@scale": _np(rows.abs().mean().reshape(1)) + 1e-30, "dlogits": _np(dl.reshape(-1, c.NB))}


@dataclass(frozen=True)
class ImagAcCase:
    N: int
    H: int
    H1: int
    NB: int = 255

    @property
    def name(self):
        return f"N{self.N}-H{self.H}-H1{self.H1}"


IMAG_AC_CASES = [ImagAcCase(1, 1, 2), ImagAcCase(5, 3, 4), ImagAcCase(67, 2, 5)]
IMAG_AC = {c.name: c for c in IMAG_AC_CASES}
AC_COEF, AC_SP, AC_SV, AC_GP, AC_GV = 3e-4, 2.0, 0.5, 0.7, -1.3


@functools.lru_cache(maxsize=None)
def imag_ac_inputs(c):
    g = _g(1000 * c.N + 10 * c.H + c.H1)
    bins = bins_f32(c.NB)
    HN = c.H * c.N
    return {"bins": bins, "vl": _peaked_logits(HN, c.NB, g) * 0.5, "logpi": torch.randn(HN, generator=g),
            "ent": torch.rand(HN, generator=g) + 0.5, "ret": _targets(bins, HN, g).view(c.N, c.H),
            "slow": _targets(bins, HN, g).flip(0).view(c.H, c.N), "weight": torch.rand(c.N, c.H1, generator=g),
            "val": torch.randn(c.H1, c.N, generator=g) * 30, "scale": torch.tensor(7.5)}


def ref_imag_ac(c, dt=F64, fault=None):
    """dreamer.py:623-671 on H * N time-major rows (the formulation of test_gpu_ops.test_imag_ac_loss_fused), the
    weights (N, H1) and values (H1, N) wider than H. Gradients of AC_GP * AC_SP * policy + AC_GV * AC_SV * value."""
    i = imag_ac_inputs(c)
    N, H = c.N, c.H
    bins = i["bins"].to(dt)
    with sm.oracle_dtype(dt):
        vl, lp, en = (i[k].to(dt).requires_grad_() for k in ("vl", "logpi", "ent"))
        ret, w = i["ret"].to(dt), i["weight"].to(dt)[:, :H]
        adv = (ret - i["val"].to(dt)[:H].t()) / i["scale"].to(dt)
        rows_p = w * -(lp.view(H, N).t() * adv + AC_COEF * en.view(H, N).t())
        lt = twohot_logp(vl, bins, ret.t().reshape(-1), fault)
        ls = twohot_logp(vl, bins, i["slow"].to(dt).reshape(-1), fault)
        rows_v = w * (-lt - ls).view(H, N).t()
        pol, val = rows_p.mean(), rows_v.mean()
        dvl, dlp, den = torch.autograd.grad(AC_GP * AC_SP * pol + AC_GV * AC_SV * val, (vl, lp, en))
    tm = lambda r: _np(r.t().reshape(-1))  # noqa: E731  (n, t) -> time-major rows t * N + n
    return {"rows_v": tm(rows_v), "rows_p": tm(rows_p), "adv": _np(adv), "policy": _np(pol.reshape(1)),
            "value": _np(val.reshape(1)), "policy@scale": _np(rows_p.abs().mean().reshape(1)) + 1e-30,
            "value@scale": _np(rows_v.abs().mean().reshape(1)) + 1e-30, "dvl": _np(dvl), "dlogpi": _np(dlp),
            "dent": _np(den)}


# =============================================================================================== pointwise heads
@dataclass(frozen=True)
class BnCase:
    rows: int
    A: int

    @property
    def name(self):
        return f"r{self.rows}-A{self.A}"


BN_CASES = [BnCase(r, a) for a in (1, 6, 16) for r in (1, 257)]
BN = {c.name: c for c in BN_CASES}
BN_MIN_STD, BN_MAX_STD = 0.1, 1.0


@functools.lru_cache(maxsize=None)
def bn_inputs(c):
    g = _g(31 * c.rows + c.A)
    a = torch.randn(c.rows, c.A, generator=g) * 1.5
    a[0, 0] = 2.5 if c.rows == 1 else -2.5  # |action| > 1: outside the mean's tanh range
    return {"x": 1.5 * torch.randn(c.rows, 2 * c.A, generator=g), "action": a,
            "glogp": torch.randn(c.rows, generator=g), "gent": torch.randn(c.rows, generator=g)}


def ref_bnormal(c, dt=F64, fault=None):
    """bounded normal log_prob / entropy (oracle bounded_normal_params, normal_log_prob, normal_entropy)"""
    i = bn_inputs(c)
    with sm.oracle_dtype(dt):
        x = i["x"].to(dt).requires_grad_()
        loc, sc = R.bounded_normal_params(x, BN_MIN_STD, BN_MAX_STD)
        lp, ent = R.normal_log_prob(loc, sc, i["action"].to(dt)), R.normal_entropy(sc)
        d_lp = torch.autograd.grad(lp, x, i["glogp"].to(dt), retain_graph=True)[0]
        d_ent = torch.autograd.grad(ent, x, i["gent"].to(dt))[0]
        # Σ|terms| with the cancellations a float32 evaluation has: d = a - loc (|a| + 1), 1 - loc^2 and 1 - sigmoid
        # (each an absolute rounding of 1), so the chain factors enter as 1 and sigmoid, not as the small differences
        xd, a = x.detach(), i["action"].to(dt)
        sc, D = sc.detach(), a.abs() + 1
        sg = torch.sigmoid(xd[:, c.A:] + 2.0)
        gl, ge = i["glogp"].to(dt).abs()[:, None], i["gent"].to(dt).abs()[:, None]
        c0 = 0.5 * np.log(2 * np.pi)
        s_lp = (D * D / (2 * sc * sc) + sc.log().abs() + c0).sum(-1)
        s_ent = (0.5 + c0 + sc.log().abs()).sum(-1)
        up = (BN_MAX_STD - BN_MIN_STD) * sg
        s_dlp = torch.cat([gl * D / (sc * sc), gl * (D * D / sc ** 3 + 1 / sc) * up], -1)
        s_dent = torch.cat([torch.zeros_like(sc), ge / sc * up], -1) + 1e-30
    return {"logp": _np(lp), "ent": _np(ent), "dx_both": _np(d_lp + d_ent), "dx_lp": _np(d_lp), "dx_ent": _np(d_ent),
            "logp@scale": _np(s_lp), "ent@scale": _np(s_ent), "dx_both@scale": _np(s_dlp + s_dent),
            "dx_lp@scale": _np(s_dlp) + 1e-30, "dx_ent@scale": _np(s_dent)}


BERN_ROWS = (1, 257)


@functools.lru_cache(maxsize=None)
def bern_inputs(rows):
    g = _g(rows)
    lo = torch.randn(rows, generator=g) * 3
    edge = torch.tensor([-40.0, 40.0, -20.0, 20.0, 0.0, -40.0, 40.0])
    v = (torch.rand(rows, generator=g) > 0.3).float()
    if rows >= 7:
        lo[:7] = edge
        v[:7] = torch.tensor([1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0])
    else:
        lo[0], v[0] = -40.0, 1.0
    return {"logit": lo, "value": v, "g": torch.randn(rows, generator=g)}


def ref_bernoulli(rows, dt=F64, fault=None):
    """torchd.Bernoulli(logits): log_prob (oracle bernoulli_log_prob) and mean = sigmoid(logits)"""
    i = bern_inputs(rows)
    with sm.oracle_dtype(dt):
        l = i["logit"].to(dt).requires_grad_()
        lp = R.bernoulli_log_prob(l.unsqueeze(-1), i["value"].to(dt).unsqueeze(-1))
        dl = torch.autograd.grad(lp, l, i["g"].to(dt))[0]
    return {"logp": _np(lp), "mean": _np(torch.sigmoid(l.detach())), "dlogit": _np(dl)}


@dataclass(frozen=True)
class GruCase:
    M: int
    G: int
    Dg: int

    @property
    def name(self):
        return f"M{self.M}-G{self.G}-Dg{self.Dg}"


GRU_CASES = [GruCase(1, 1, 64), GruCase(3, 8, 96), GruCase(37, 2, 512)]
GRU = {c.name: c for c in GRU_CASES}


@functools.lru_cache(maxsize=None)
def gru_inputs(c):
    g = _g(c.M + c.G + c.Dg)
    D = c.G * c.Dg
    return {"gates": torch.randn(c.M, 3 * D, generator=g) * 2, "h": torch.randn(c.M, D, generator=g),
            "dout": torch.randn(c.M, D, generator=g), "dh0": torch.randn(c.M, D, generator=g)}


def ref_gru(c, dt=F64, fault=None):
    """Deter gates (rssm.py:65-75): r = sigmoid, c = tanh(r * c), u = sigmoid(u - 1), h' = u c + (1 - u) h, the gates
    (M, G, 3, Dg) — the restatement of test_gpu_ops.test_gru_gates."""
    i = gru_inputs(c)
    gt, h = i["gates"].to(dt).requires_grad_(), i["h"].to(dt).requires_grad_()
    r, cc, u = (t.reshape(c.M, -1) for t in torch.chunk(gt.view(c.M, c.G, -1), 3, -1))
    r = torch.sigmoid(r)
    cc = torch.tanh(r * cc)
    u = torch.sigmoid(u - 1)
    out = u * cc + (1 - u) * h
    dg, dh = torch.autograd.grad(out, (gt, h), i["dout"].to(dt))
    return {"out": _np(out), "dgates": _np(dg), "dh": _np(dh), "dh_acc": _np(dh + i["dh0"].to(dt))}


# =============================================================================================== λ-return
@dataclass(frozen=True)
class LretCase:
    N: int
    T: int
    form: str  # replay (term, last, boot of its own) | imag (cont_logit, cont_out, weight_out) | both (term + cont_logit)
    lamb: float = LAMB

    @property
    def name(self):
        return f"N{self.N}-T{self.T}-{self.form}" + (f"-lamb{self.lamb:g}" if self.lamb != LAMB else "")

    def arm(self):
        return lret_arm(self.T, self.form != "imag", self.form != "replay")


LRET_CASES = ([LretCase(n, t, f) for n, t in ((1, 1), (1, 2), (17, 5), (33, 64), (17, 255), (17, 256))
               for f in ("replay", "imag")]
              + [LretCase(3, 5, "both")] + [LretCase(17, 5, f, l) for l in (0.0, 1.0) for f in ("replay", "imag")])
LRET = {c.name: c for c in LRET_CASES}
assert len(LRET) == len(LRET_CASES)


@functools.lru_cache(maxsize=None)
def lret_inputs(c):
    g = _g(1000 * c.N + c.T)
    sh = (c.N, c.T)
    d = {"reward": torch.randn(sh, generator=g), "value": torch.randn(sh, generator=g) * 5,
         "boot": torch.randn(sh, generator=g) * 5, "cont_logit": torch.randn(sh, generator=g) * 2,
         "term": (torch.rand(sh, generator=g) < 0.15).float(), "last": (torch.rand(sh, generator=g) < 0.15).float()}
    if c.T >= 2:  # rows with last alone, term alone and both, at a step the return reads (t >= 1)
        for r, (la, te) in enumerate(((1.0, 0.0), (0.0, 1.0), (1.0, 1.0))[:c.N]):
            d["last"][r, c.T // 2 if c.T > 2 else 1], d["term"][r, c.T // 2 if c.T > 2 else 1] = la, te
        if c.N == 1:
            d["last"][0, 1], d["term"][0, 1] = 1.0, 0.0
    return d


def ref_lret(c, dt=F64, fault=None):
    """Dreamer._lambda_return (oracle lambda_return, ref_cpu.py:578-585); imagination form: term = 1 - sigmoid(logit),
    last = 0, boot = value, cont / weight = sigmoid, cumprod(cont * disc) (dreamer.py:590-599).
    faults: "last_ignored", "term_at_t" (term read at t instead of t + 1)."""
    i = lret_inputs(c)
    out = {}
    with sm.oracle_dtype(dt):
        rew = i["reward"].to(dt)
        cont = torch.sigmoid(i["cont_logit"].to(dt))
        term = i["term"].to(dt) if c.form != "imag" else 1 - cont
        last = i["last"].to(dt) if c.form != "imag" else torch.zeros_like(rew)
        boot = i["boot"].to(dt) if c.form != "imag" else i["value"].to(dt)
        # T = 2: ret[0] = r[1] + live ((1 - cnt) + cnt) boot[1], whatever last is: the fault cannot change it
        if fault == "last_ignored" and c.T > 2:
            last = torch.zeros_like(last)
        if fault == "term_at_t":
            term = torch.cat([term[:, :1], term[:, :-1]], 1)
        if c.T == 1:  # the return covers steps 0 .. T - 2: empty
            out["ret"] = np.zeros((c.N, 0), _np(rew).dtype)
        else:
            out["ret"] = _np(R.lambda_return(last, term, rew, boot, boot, DISC, c.lamb)).reshape(c.N, c.T - 1)
        if c.form != "replay":
            out["cont"], out["weight"] = _np(cont), _np(torch.cumprod(cont * DISC, 1))
    return out


# =============================================================================================== ReturnEMA
EMA_NS = (1, 2, 21, 1000, 16384, 16385, 40001)
EMA_KINDS = ("normal10", "constant", "two_values", "ties", "zeros_mix")
EMA0 = (0.3, 1.2)
EMA_ALPHA = 1e-2


@dataclass(frozen=True)
class EmaCase:
    n: int
    kind: str

    @property
    def name(self):
        return f"n{self.n}-{self.kind}"


EMA_CASES = [EmaCase(n, k) for n in EMA_NS for k in EMA_KINDS]
EMA = {c.name: c for c in EMA_CASES}


@functools.lru_cache(maxsize=None)
def ema_inputs(c):
    """two inputs: the second call continues from the first's in-place EMA"""
    def one(seed):
        g = _g(seed)
        z = torch.randn(c.n, generator=g)
        if c.kind == "normal10":
            return z * 10
        if c.kind == "constant":
            return torch.full((c.n,), 0.75 + seed % 2)
        if c.kind == "two_values":
            return torch.where(z > 0.3, torch.tensor(2.5), torch.tensor(-1.25))
        if c.kind == "ties":
            return torch.round(z * 10) / 10
        x = z.clone()  # zeros_mix: a third +0.0, a third -0.0, the rest as drawn (half negative)
        x[0::3], x[1::3] = 0.0, -0.0
        return x
    return {"x1": one(3 * c.n + 1), "x2": one(3 * c.n + 2)}


def quantiles_f32(x, fault=None):
    """torch.quantile(x, [0.05, 0.95]) on the float32 CPU tensor: exact selection + torch's lerp; the kernel is compared
    bit for bit with it. fault "nearest_rank": no interpolation."""
    q = torch.tensor([0.05, 0.95])
    return torch.quantile(x, q, interpolation="nearest" if fault == "nearest_rank" else "linear")


def ref_ema(c, dt=F64, fault=None):
    """ReturnEMA.__call__ (networks.py:416-422; oracle return_ema, ref_cpu.py:588-592), twice. faults: "nearest_rank",
    "ema_not_carried" (the second call starts from the initial EMA again)."""
    i = ema_inputs(c)
    ema = torch.tensor(EMA0, dtype=dt)
    out = {}
    for k in ("1", "2"):
        q = quantiles_f32(i["x" + k], fault)
        if fault == "ema_not_carried":
            ema = torch.tensor(EMA0, dtype=dt)
        sc = (EMA_ALPHA * q.to(dt)).abs() + ((1 - EMA_ALPHA) * ema).abs()  # the two terms of the EMA
        ema = EMA_ALPHA * q.to(dt) + (1 - EMA_ALPHA) * ema
        out["q" + k], out["ema" + k] = _np(q), _np(ema)
        out["os" + k] = _np(torch.stack([ema[0], torch.clip(ema[1] - ema[0], min=1.0)]))
        out["ema" + k + "@scale"] = _np(sc)
        out["os" + k + "@scale"] = _np(torch.stack([sc[0], sc.sum() + 1.0]))
    return out


# =============================================================================================== registry
# family -> (cases, reference(case, dt, fault)); RMSNorm runs per act
FAMILIES = {
    "rms": (RMS_CASES, None),
    "colsum": (COLSUM_CASES, ref_colsum),
    "sample": (TEAM_CASES, ref_sample),
    "logp": (TEAM_CASES, ref_logp),
    "kl": (KL_CASES, ref_kl),
    "twohot": (TWOHOT_CASES, ref_twohot),
    "repval": (REPVAL_CASES, ref_repval),
    "imag_ac": (IMAG_AC_CASES, ref_imag_ac),
    "bnormal": (BN_CASES, ref_bnormal),
    "bernoulli": (BERN_ROWS, ref_bernoulli),
    "gru": (GRU_CASES, ref_gru),
    "lret": (LRET_CASES, ref_lret),
    "ema": (EMA_CASES, ref_ema),
}
FAULTS = {
    "rms": ("rms_padded_mean", "dw_first_stride", "acc_dx_ignored"),
    "colsum": ("colsum_drop_tail",),
    "sample": ("unimix_omitted",),
    "logp": ("unimix_omitted",),
    "kl": ("kl_grad_below_free", "kl_s_minus_1"),
    "twohot": ("twohot_swapped",),
    "repval": ("repval_row_stride",),
    "imag_ac": ("twohot_swapped",),
    "lret": ("last_ignored", "term_at_t"),
    "ema": ("nearest_rank", "ema_not_carried"),
}


@functools.lru_cache(maxsize=None)
def reference(fam, case, act=None):
    """the float64 reference, computed once and shared"""
    if fam == "rms":
        return ref_rms(case, act)
    return FAMILIES[fam][1](case)
