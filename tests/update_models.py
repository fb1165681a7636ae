"""Cases, inputs, float64 references and comparisons for the tail of the update: csrc/misc.hip (Barlow, InfoNCE, the
metric vector, the weighted loss total, input preparation, replay slices) and csrc/optim.hip (AGC + LaProp, Polyak).
Test infrastructure (a plain module: no fixtures, no pytest hooks), in the pattern of rowop_models.py.

Shared by tests/test_update_parity_cpu.py (the tables reach every dispatch arm, the input conditions hold, the float32
restatement passes every comparison with room, planted faults fail it) and tests/test_gpu_update_f64.py (the kernels
against float64). DESIGN.md § 2.4 holds the tables and the measured figures.

A reference is one function `ref_<family>(case, dt, fault)`: the oracle's own functions (oracle/ref_cpu.py, its
arithmetic type switched by small_models.oracle_dtype: symlog, tensorstats, OracleAgent.agc_ / laprop_step / lr /
update_slow_target) or, where the oracle has none, a torch restatement of the reference's expression, evaluated in
`dt`. dt = float64 is the reference, dt = float32 the restatement whose distance from float64 sizes the tolerances,
`fault` plants one named error. It returns {output: ndarray}; an output that is a sum also returns `output@scale`,
the Σ|terms| of each element, and an output with a rounding no evaluation avoids `output@floor`.

Comparison (compare / ratios): every output elementwise through parity.assert_close with rtol = 0 and
  atol_i = tol * max(|ref_i|, 1)                    for a pointwise output ("pt"),
  atol_i = k * eps32 * scale_i (+ floor_i)          for a sum ("sum"; scale_i = the float64 Σ|terms| of that element),
  atol_i = tol * ulp32(mag_i)                       for a value of one or two roundings ("ulp"),
  atol_i = tol * |ref_i|                            for the float64 scalar state ("rel"),
and, beside it, the existing tests' figure in the existing tests' own form as a cap (Tol.form). Copies, selections,
indices, min and max are compared exactly.
"""
import functools
import types
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

import parity
import small_models as sm
from oracle import ref_cpu as R
from rowop_models import EPS32, F32, F64, _g, _np, outputs, same_bits  # noqa: F401  (one net: the same helpers)


# =============================================================================================== tolerances
@dataclass(frozen=True)
class Tol:
    cap: float  # the existing tests' figure, in the existing tests' form (`form`); never loosened
    tol: float
    kind: str = "pt"  # "pt" | "sum" | "ulp" | "rel" | "exact"
    form: str = "max"  # max: close(); allclose: rtol = cap, atol 1e-6; delta; moment; ulp; none
    capped: bool = False  # the tolerance is the cap itself (8 x the measured distance exceeds it)


EXACT = Tol(0.0, 0.0, "exact", "none")


def _sum(cap, k, form="max", capped=False):
    return Tol(cap, k, "sum", form, capped)


# Each tolerance is 8 x the larger of two measured distances from float64, in the output's own unit (units()): the
# float32 restatement's on the CPU and the kernel's on the MI355X (DESIGN.md § 2.4 lists all three per output). Where
# that exceeds the cap, the cap is the tolerance.
TOL = {
    "barlow": {
        "mean": _sum(1e-5, 12.0), "std": _sum(1e-5, 13.0), "sums": _sum(1e-5, 12.0), "q": _sum(1e-5, 16.0),
        "craw": _sum(1e-5, 22.0), "d1": Tol(1e-6, 1e-6, capped=True), "d2": Tol(1e-6, 1e-6, capped=True),
        "n1": Tol(1e-5, 2e-6), "n2": Tol(1e-5, 2.2e-6), "c": _sum(1e-5, 25.0), "z2": _sum(1e-4, 11.0),
        "loss": _sum(1e-5, 5.0), "dc": _sum(1e-5, 21.0), "dx1": _sum(1e-5, 63.0), "s0": _sum(1e-5, 15.0),
        "A": _sum(1e-5, 19.0), "sbwd": _sum(1e-5, 14.0), "s0d": _sum(1e-5, 5.1), "Ad": _sum(1e-5, 5.1),
        "dxd": _sum(1e-5, 13.1)},
    "infonce": {"lse": _sum(1e-5, 6.8), "row_loss": _sum(1e-5, 8.3), "loss": _sum(1e-5, 4.1),
                "dlogits": _sum(1e-5, 23.0), "fn_loss": _sum(1e-5, 2.7), "dx1": _sum(1e-5, 7.3)},
    "stats": {"mean": _sum(2e-6, 5.8, "allclose"), "std": _sum(2e-6, 4.6, "allclose"), "min": EXACT, "max": EXACT,
              "affine": _sum(2e-6, 5.8, "allclose"), "affine_std": _sum(2e-6, 4.3, "allclose"),
              "combo": _sum(2e-6, 4.1, "allclose"), "nan": EXACT},
    "loss_terms": {"means": _sum(1e-6, 2.7), "total": _sum(1e-6, 0.85), "grads": _sum(1e-6, 6.8)},
    # action_norm is exact in every type: a / 1 = a, a / |a| = +-1. The u8 kernels: the issue's 1 float32 ulp, which
    # two correctly rounded operations of half an ulp each fill (no 8 x: IEEE's bound, not a measured distance)
    "prep": {"symlog": _sum(1e-6, 3.8), "action_norm": EXACT, "mask_rows": EXACT, "last": EXACT,
             "term": EXACT, "cont": EXACT, "u8": Tol(1.0, 1.0, "ulp", "ulp", True),
             "img": Tol(1.0, 1.0, "ulp", "ulp", True), "enc": Tol(1.0, 1.0, "ulp", "ulp", True),
             "pad": Tol(1.0, 1.0, "ulp", "ulp", True), "u8_f32": EXACT, "img_f32": EXACT, "enc_f32": EXACT,
             "pad_f32": EXACT},
    "optim": {"dp": _sum(1e-4, 21.0, "delta"), "m": _sum(1e-5, 28.0, "moment"), "v": _sum(1e-5, 66.0, "moment"),
              "gn": _sum(1e-5, 4.9, "none"), "scalars": Tol(1e-12, 1e-12, "rel", "none")},
    # test_polyak's 1 ulp is a distance between two float32 evaluations (asserted as such in the GPU test); against
    # float64 the two products' and the sum's roundings are the floor wherever the terms cancel (645 ulp of the result
    # at n = 100003), so here the update is a sum of its two terms
    "polyak": {"dst": _sum(1.0, 9.0, "none")},
    "slices": {},
}
for _fam in TOL.values():
    assert all(t.kind != "pt" or t.tol <= t.cap for t in _fam.values())


def base_name(fam, name):
    """the TOL entry of an output: its own name, the name without a step number (dp0, dp1, ...), or its prefix
    (grads_all, enc_c3p4s0.5, mask_rows_w7s3)"""
    T = TOL[fam]
    if name in T:
        return name
    if name.rstrip("0123456789") in T:
        return name.rstrip("0123456789")
    for k in sorted(T, key=len, reverse=True):
        if name.startswith(k + "_"):
            return k
    return name


def tol_of(fam, name):
    return TOL[fam].get(base_name(fam, name), EXACT)


def _atol(t, ref, name):
    r = np.asarray(ref[name], np.float64)
    if t.kind == "sum":
        a = t.tol * EPS32 * np.asarray(ref[name + "@scale"], np.float64)
    elif t.kind == "ulp":
        a = t.tol * parity.ulp(ref.get(name + "@mag", r))
    elif t.kind == "rel":
        a = t.tol * np.abs(r)
    else:
        a = t.tol * np.maximum(np.abs(r), 1.0)
    if name + "@floor" in ref:
        a = a + np.asarray(ref[name + "@floor"], np.float64)
    return a


def _cap_ratio(t, got, r, ref, name):
    """the existing tests' check, in its own form: the fraction of it used"""
    if t.form == "none" or r.size == 0:
        return 0.0
    err = np.abs(got - r)
    tiny = 1e-300
    if t.form == "max":  # test_gpu_ops.close()
        v = err.max() / (t.cap * max(np.abs(r).max(), 1.0))
    elif t.form == "allclose":  # test_metric_vector: rtol 2e-6, atol 1e-6
        v = (err / (t.cap * np.abs(r) + 1e-6)).max()
    elif t.form == "delta":  # test_laprop_agc_step: 1e-4 |dp_ref| + 4 ulp(p)
        v = (err / np.maximum(t.cap * np.abs(r) + 4 * ref[name + "@ulp"], tiny)).max()
    elif t.form == "moment":  # test_laprop_agc_step: 1e-5 |b| + 1e-5 max|b| per tensor
        v = 0.0
        for lo, hi in ref["@seg"]:
            b = np.abs(r[lo:hi])
            v = max(v, float((err[lo:hi] / np.maximum(t.cap * b + t.cap * b.max(), tiny)).max()))
    elif t.form == "ulp":  # test_polyak / one rounding
        v = (err / (t.cap * parity.ulp(ref.get(name + "@mag", r)))).max()
    else:
        raise ValueError(t.form)
    return float(np.nan_to_num(v, nan=np.inf))


def _pair(got, ref, name):
    g, r = np.asarray(got[name]), np.asarray(ref[name])
    assert g.shape == r.shape, (name, g.shape, r.shape)
    return g, r


def ratios(fam, got, ref):
    """{output: (fraction of the elementwise bound used, fraction of the cap used)}; exact outputs: 0 or inf"""
    out = {}
    for name in outputs(ref):
        if name not in got:
            continue
        t = tol_of(fam, name)
        g, r = _pair(got, ref, name)
        if t.kind == "exact":
            out[name] = (0.0 if np.array_equal(g, r, equal_nan=g.dtype.kind == "f") else float("inf"),) * 2
        else:
            g, r = g.astype(np.float64), r.astype(np.float64)
            # a floor (a rounding no evaluation avoids) is reached, not approached: the fraction is of what is above it
            fl = np.asarray(ref.get(name + "@floor", 0.0), np.float64)
            free = {k: v for k, v in ref.items() if k != name + "@floor"}
            a = parity.bound_ratio(np.maximum(np.abs(g - r) - fl, 0.0), 0 * r, 0.0, _atol(t, free, name))
            out[name] = (float(np.nan_to_num(a, nan=np.inf)), _cap_ratio(t, g, r, ref, name))
    return out


def units(fam, got, ref):
    """{output: max error in the output's own unit}: the figure a tolerance is chosen from (times 8, inside the cap).
    A floor (a rounding no evaluation avoids) is taken off first."""
    out = {}
    for name in outputs(ref):
        t = tol_of(fam, name)
        if name not in got or t.kind == "exact" or np.asarray(ref[name]).size == 0:
            continue
        g, r = _pair(got, ref, name)
        g, r = g.astype(np.float64), r.astype(np.float64)
        one = _atol(Tol(t.cap, 1.0, t.kind, t.form), {k: v for k, v in ref.items() if k != name + "@floor"}, name)
        err = np.maximum(np.abs(g - r) - np.asarray(ref.get(name + "@floor", 0.0)), 0.0)
        key = base_name(fam, name)
        out[key] = max(out.get(key, 0.0), float((err / np.maximum(one, 1e-300)).max()))
    return out


def summary(rt):
    return " ".join(f"{k}={a:.2g}/{b:.2g}" for k, (a, b) in rt.items())


def compare(fam, got, ref, what=""):
    for name in outputs(ref):
        if name not in got:
            continue
        t = tol_of(fam, name)
        g, r = _pair(got, ref, name)
        if t.kind == "exact":
            same = np.array_equal(g, r, equal_nan=g.dtype.kind == "f")
            assert same, f"{what} {name}: {int((g != r).sum())} of {r.size} differ"
            continue
        if r.size == 0:
            continue
        g, r = g.astype(np.float64), r.astype(np.float64)
        assert np.isfinite(g).all(), f"{what} {name}: not finite"
        parity.assert_close(g, r, 0.0, _atol(t, ref, name), f"{what} {name}")
        cr = _cap_ratio(t, g, r, ref, name)
        assert cr <= 1.0, f"{what} {name}: {cr:.3g} of the cap {t.cap} ({t.form})"


def passes(fam, got, ref):
    return all(a <= 1.0 and b <= 1.0 for a, b in ratios(fam, got, ref).values())


# =============================================================================================== Barlow
CS_NP = 16  # misc.hip:82
BARLOW_LAMBD, BARLOW_EPS, BARLOW_G = 5e-4, 1e-8, 0.7
BARLOW_MIN_STD = 0.5
BARLOW_PARTIAL_BLOCKS = 256  # ops.py:867 / parallel.py:170: `nblocks` of sd_barlow_loss


def col_blocks(C):
    """misc.hip:85, 649: 64 columns per workgroup; (blocks, columns of the last one)"""
    nb = (C + 63) // 64
    return nb, C - 64 * (nb - 1)


def row_partials(R_):
    """misc.hip:91: partial `part` sums rows part, part + 16, ...: (rows of the fullest partial, partials with one row
    fewer)"""
    full = -(-R_ // CS_NP)
    return full, (CS_NP - R_ % CS_NP) % CS_NP


def barlow_partial_strides(E, nblocks=BARLOW_PARTIAL_BLOCKS):
    """misc.hip:175: i = block * 256 + thread, stride nblocks * 256 over E * E elements"""
    return -(-E * E // (nblocks * 256))


def rowstats_blocks(E):
    """misc.hip:267-268, 693: a wave per row, 4 rows per workgroup; (blocks, idle waves of the last one)"""
    nb = (E + 3) // 4
    return nb, 4 * nb - E


@dataclass(frozen=True)
class BarlowCase:
    Nr: int
    E: int
    mode: str  # fn: ops.BarlowFn | w1: parallel.BarlowSteps at world 1 | sh: two simulated shards
    split: object = None  # sh: the shards' rows (default two halves)

    @property
    def name(self):
        return f"{self.mode}-{self.Nr}x{self.E}" + (f"-{self.split[0]}+{self.split[1]}" if self.split else "")

    def shards(self):
        if self.mode != "sh":
            return (self.Nr,)
        return tuple(self.split) if self.split else (self.Nr // 2, self.Nr // 2)

    @property
    def world(self):
        return len(self.shards())


BARLOW_NR, BARLOW_E = (2, 16, 17, 33), (1, 5, 64, 65, 257)
BARLOW_CASES = ([BarlowCase(n, e, m) for m in ("fn", "w1") for n in BARLOW_NR for e in BARLOW_E]
                + [BarlowCase(n, e, "sh") for n in (2, 16) for e in BARLOW_E]
                + [BarlowCase(17, 65, "sh", (5, 12))]
                + [BarlowCase(512, 1024, m) for m in ("fn", "w1", "sh")])
BARLOW = {c.name: c for c in BARLOW_CASES}
assert len(BARLOW) == len(BARLOW_CASES)
BARLOW_OUTPUTS = {
    "fn": ("mean", "std", "n1", "n2", "c", "loss", "dc", "dx1", "sbwd"),
    "w1": ("sums", "d1", "d2", "q", "craw", "c", "std", "n2", "z2", "loss", "dc", "s0", "A", "dx1", "s0d", "Ad", "dxd"),
}
BARLOW_OUTPUTS["sh"] = BARLOW_OUTPUTS["w1"]


def _spread_columns(x):
    """every column's float64 std >= 0.5 + margin: a narrow column gets its first row moved off the others' mean"""
    N = x.shape[0]
    sd = x.double().std(0)
    bad = sd < BARLOW_MIN_STD + 0.25
    if bool(bad.any()):
        rest = x[1:].double().mean(0)
        x[0] = torch.where(bad, (rest + max(2.0, N ** 0.5)).float(), x[0])
    return x


@functools.lru_cache(maxsize=None)
def barlow_inputs(c):
    g = _g(7919 * c.Nr + c.E)
    N, E = c.Nr, c.E
    x1 = _spread_columns(torch.randn(N, E, generator=g) * 2 + 0.5)
    x2 = _spread_columns(torch.randn(N, E, generator=g) - 0.25)
    d = {"x1": x1, "x2": x2, "dnr": torch.randn(N, E, generator=g)}
    if c.mode != "fn":  # the backward's reductions on inputs of their own: z2 and the row sums are ~0 in the pipeline
        d.update(dcr=torch.randn(E, E, generator=g), cr=torch.randn(E, E, generator=g) * 0.3,
                 z2r=torch.randn(E, generator=g), s1r=torch.rand(E, generator=g) + 0.5,
                 s0r=torch.randn(E, generator=g), Ar=torch.randn(E, generator=g),
                 sums_in=torch.stack([x1.double().sum(0), x2.double().sum(0)]).float())
    return d


def ref_barlow(c, dt=F64, fault=None):
    """dreamer.py:525-532 (oracle ref_cpu.py:722-728): x_n = (x - mean) / (std + 1e-8), c = x1n^T x2n / N,
    loss = sum_i (c_ii - 1)^2 + lambd sum_{i != j} c_ij^2, its gradient to x1 for an upstream g, and every intermediate
    the kernels pass on. The mean and the unbiased std are written out as the sums they are (so a fault can be planted
    in them); the backward's reductions (misc.hip:129, 262, 282) again on inputs of their own.
    faults: "biased_std" (/ N); "mean_padded_ld" (the mean's pass reads row r at r * the 64-padded width);
    "drop_last_partial" (the rows of the last, partly filled stride of 16 left out of the column sums);
    "lambda_on_diag"; "no_mean_dn" (dx without the mean-of-dn term); "shard_R_for_Nt" (the first shard's rows for N)."""
    i = barlow_inputs(c)
    N, E = c.Nr, c.E
    lam, eps, gup = BARLOW_LAMBD, BARLOW_EPS, BARLOW_G
    Nd = float(c.shards()[0]) if fault == "shard_R_for_Nt" else float(N)
    keep = N - N % CS_NP if fault == "drop_last_partial" else N
    x1, x2 = i["x1"].to(dt).requires_grad_(), i["x2"].to(dt)

    def colsum(x):
        if fault == "mean_padded_ld":
            C64 = 64 * col_blocks(E)[0]
            x = F.pad(x.reshape(-1), (0, N * C64 - N * E)).view(N, C64)[:, :E]
        return x[:keep].sum(0)

    def stats(x):
        s = colsum(x)
        d = x - s / Nd
        q = (d[:keep] * d[:keep]).sum(0)
        return s, d, q, torch.sqrt(q / (Nd if fault == "biased_std" else Nd - 1.0))

    su1, d1, q1, s1 = stats(x1)
    su2, d2, q2, s2 = stats(x2)
    n1, n2 = d1 / (s1 + eps), d2 / (s2 + eps)
    cc = torch.mm(n1.t(), n2) / Nd
    eye = torch.eye(E, dtype=torch.bool)
    inv = (torch.diagonal(cc) - 1.0).pow(2).sum()
    red = cc[~eye].pow(2).sum()
    loss = (lam * inv if fault == "lambda_on_diag" else inv) + lam * red
    dc, dx1 = torch.autograd.grad(loss, (cc, x1), torch.tensor(gup, dtype=dt), retain_graph=True)
    dnr = i["dnr"].to(dt)
    if fault == "no_mean_dn":
        with torch.no_grad():
            sc = s1 + eps
            sbwd = dnr / sc - d1 * ((dnr * d1).sum(0) / (sc * sc * (Nd - 1.0) * s1))
    else:
        sbwd = torch.autograd.grad(n1, x1, dnr)[0]
    with torch.no_grad():
        dn1 = torch.mm(n2, dc.t()) / Nd
        out = {"mean": torch.stack([su1, su2]) / Nd, "std": torch.stack([s1, s2]), "sums": torch.stack([su1, su2]),
               "d1": d1, "d2": d2, "q": torch.stack([q1, q2]), "craw": torch.mm(d1.t(), d2), "n1": n1, "n2": n2,
               "c": cc, "z2": n2.sum(0), "loss": loss.reshape(1), "dc": dc, "dx1": dx1, "s0": dn1.sum(0),
               "A": (dn1 * d1).sum(0), "sbwd": sbwd}
        # Σ|terms|, first order: c's terms are n1 n2 / N (the roundings of n enter k); the loss and dc carry c's
        # error through 2 w |c - I|; dn1 = n2 dc^T / N carries dc's; dx1, s0 and A carry dn1's
        a1, a2 = x1.abs().sum(0), x2.abs().sum(0)
        w = torch.where(eye, torch.ones((), dtype=dt), torch.tensor(lam, dtype=dt))
        Sc = torch.mm(n1.abs().t(), n2.abs()) / Nd
        cm = (cc - eye.to(dt)).abs()
        S_dc = abs(gup) * 2 * w * Sc + dc.abs()
        S_dn = torch.mm(n2.abs(), S_dc.t()) / Nd
        sc1, dm = s1 + eps, d1.abs()
        k2 = sc1 * sc1 * (Nd - 1.0) * s1
        out.update({"mean@scale": torch.stack([a1, a2]) / Nd, "sums@scale": torch.stack([a1, a2]),
                    "std@scale": out["std"], "q@scale": out["q"], "craw@scale": torch.mm(dm.t(), d2.abs()),
                    "c@scale": Sc, "z2@scale": n2.abs().sum(0),
                    "loss@scale": ((w * cm * cm).sum() + (2 * w * cm * Sc).sum()).reshape(1), "dc@scale": S_dc,
                    "dx1@scale": (S_dn + S_dn.mean(0)) / sc1 + dm * ((S_dn * dm).sum(0) / k2),
                    "s0@scale": S_dn.sum(0), "A@scale": (S_dn * dm).sum(0),
                    "sbwd@scale": (dnr.abs() + dnr.abs().mean(0)) / sc1 + dm * ((dnr.abs() * dm).sum(0) / k2)})
        if c.mode != "fn":
            dcr, cr, z2r, s1r, s0r, Ar, sums = (i[k].to(dt) for k in ("dcr", "cr", "z2r", "s1r", "s0r", "Ar", "sums_in"))
            scr = s1r + eps
            m1 = sums[0] / Nd
            kk = Ar / (scr * scr * (Nd - 1.0) * s1r)
            mdn = 0.0 if fault == "no_mean_dn" else s0r / Nd
            x1d = x1.detach()
            out.update({"s0d": (dcr * z2r).sum(1) / Nd, "s0d@scale": (dcr * z2r).abs().sum(1) / Nd,
                        "Ad": scr * (dcr * cr).sum(1), "Ad@scale": scr * (dcr * cr).abs().sum(1),
                        "dxd": ((dnr - mdn) / scr - (x1d - m1) * kk) * c.world,
                        "dxd@scale": ((dnr.abs() + s0r.abs() / Nd) / scr + (x1d.abs() + m1.abs()) * kk.abs()) * c.world})
    want = BARLOW_OUTPUTS[c.mode]
    return {k: _np(v) + (1e-30 if "@" in k else 0) for k, v in out.items() if k.split("@")[0] in want}


# =============================================================================================== InfoNCE
NCE_E = 8
NCE_G = 0.7
NCE_SHAPES = ((1, 1, 0), (3, 3, 0), (3, 7, 4), (2, 255, 0), (5, 256, 251), (5, 257, 100), (300, 600, 300))
# 80: rows reach +-80. exp(80) = 5.5e34 is still a float32 (exp overflows float32 from 88.73), so 100 is run too:
# there a float32 sum of exp without the row maximum is inf
NCE_MAGS = (0, 80, 100)
EXP_OVERFLOW_F32 = 88.7228


@dataclass(frozen=True)
class NceCase:
    n: int
    ncol: int
    off: int
    mag: int = 0
    ld_extra: int = 0

    @property
    def name(self):
        return (f"n{self.n}-c{self.ncol}-o{self.off}" + (f"-mag{self.mag}" if self.mag else "")
                + (f"-ld{self.ld_extra}" if self.ld_extra else ""))


NCE_CASES = [NceCase(*s, mag=m) for s in NCE_SHAPES for m in NCE_MAGS] + [NceCase(5, 257, 100, ld_extra=3)]
NCE = {c.name: c for c in NCE_CASES}


def nce_row_strides(ncol):
    """misc.hip:722, 729: a row's columns over 256 threads"""
    return -(-ncol // 256)


def mean_strides(n):
    """misc.hip:740 mean_kernel: n values over 256 threads"""
    return -(-n // 256)


@functools.lru_cache(maxsize=None)
def nce_inputs(c):
    g = _g(1000 * c.n + c.ncol + c.off)
    l = torch.randn(c.n, c.ncol, generator=g) * 2
    x1, x2g = torch.randn(c.n, NCE_E, generator=g), torch.randn(c.ncol, NCE_E, generator=g)
    if c.mag:
        if c.ncol == 1:
            l = torch.full((c.n, 1), float(c.mag)) * (1 - 2 * (torch.arange(c.n) % 2)).float()[:, None]
        else:
            hi, lo = l.max(1, keepdim=True).values, l.min(1, keepdim=True).values
            l = (l - (hi + lo) / 2) / ((hi - lo) / 2) * c.mag
        x1 = x1 * (c.mag / torch.mm(x1.double(), x2g.double().t()).abs().max()).float()
    return {"logits": l.contiguous(), "x1": x1, "x2g": x2g}


def _nce_rows(l, labels, fault):
    """-> (row losses, lse). oracle ref_cpu.py:732-735: cross_entropy(logits - max(logits, 1), arange)"""
    ar = torch.arange(l.shape[0])
    if fault == "no_rowmax":
        lse = torch.log(torch.exp(l).sum(1))
        return lse - l[ar, labels], lse
    nl = l - torch.max(l, 1)[0][:, None]
    return F.cross_entropy(nl, labels, reduction="none"), torch.logsumexp(l, 1)


def _nce_mean(rows, fault):
    return rows[:256].sum() / rows.shape[0] if fault == "mean_256_rows" else rows.mean()


def ref_infonce(c, dt=F64, fault=None):
    """dreamer.py:533-542 on given logits (sd_infonce_fwd / _bwd: rows, lse, their mean, dlogits for an upstream g and
    the 1 / n the mean carries) and through ops.InfoNCEFn from x1, x2g (fn_loss, dx1).
    faults: "no_rowmax"; "label_at_r" (column r, not r + off); "mean_256_rows"."""
    i = nce_inputs(c)
    n = c.n
    labels = torch.arange(n) + (0 if fault == "label_at_r" else c.off)
    l = i["logits"].to(dt).requires_grad_()
    rows, lse = _nce_rows(l, labels, fault)
    loss = _nce_mean(rows, fault)
    dl = torch.autograd.grad(rows.sum(), l)[0] * (NCE_G / n)  # the kernel: g * scale * (softmax - onehot)
    x1, x2g = i["x1"].to(dt).requires_grad_(), i["x2g"].to(dt)
    lf = torch.matmul(x1, x2g.t())
    rows_f, _ = _nce_rows(lf, labels, fault)
    fn_loss = _nce_mean(rows_f, fault)
    dx1 = torch.autograd.grad(rows_f.mean(), x1)[0] * NCE_G
    with torch.no_grad():
        def scales(lg, lse_):
            m = lg.max(1).values
            s_lse = m.abs() + (lse_ - m).abs() + 1.0  # m + log(s): two terms, and the sum of exp's relative error
            s_row = s_lse + lg[torch.arange(n), labels].abs()
            p = torch.exp(lg - lse_[:, None])
            oh = F.one_hot(labels, c.ncol).to(lg.dtype)
            # a float32 exp carries (1 + |argument|) roundings of its argument, and lse's error
            s_dl = (NCE_G / n) * (p * (1 + (lg - lse_[:, None]).abs() + s_lse[:, None]) + oh)
            return s_lse, s_row, s_dl
        ld_, lse_d = l.detach(), lse.detach()
        s_lse, s_row, s_dl = scales(ld_, lse_d)
        lfd = lf.detach()
        S_l = torch.matmul(x1.detach().abs(), x2g.abs().t())  # the GEMM's Σ|terms| per logit
        fl_lse, fl_row, fl_dl = scales(lfd, torch.logsumexp(lfd, 1))
        pf = torch.softmax(lfd, 1)
        oh = F.one_hot(labels, c.ncol).to(dt)
        row_from_l = (S_l * (pf + oh)).sum(1)  # d row / d logit = p - onehot
        # d dl / d logit: p (delta - p) -> |.| <= p per source logit, summed over the row
        dl_from_l = (NCE_G / n) * (pf * S_l + pf * (pf * S_l).sum(1, keepdim=True))
    return {"lse": _np(lse), "lse@scale": _np(s_lse), "row_loss": _np(rows), "row_loss@scale": _np(s_row),
            "loss": _np(loss.reshape(1)), "loss@scale": _np(s_row.mean().reshape(1)),
            "dlogits": _np(dl), "dlogits@scale": _np(s_dl) + 1e-30,
            "fn_loss": _np(fn_loss.reshape(1)), "fn_loss@scale": _np((fl_row + row_from_l).mean().reshape(1)),
            "dx1": _np(dx1), "dx1@scale": _np(torch.matmul(fl_dl + dl_from_l, x2g.abs())) + 1e-30}


# =============================================================================================== metric vector
STAT_CHUNK = 4096  # sdhip.h SD_STAT_CHUNK
STAT_NS = (1, 2, 4095, 4096, 4097, 3 * 4096 + 5)
STAT_SUB, STAT_DIV = 0.25, 4.0
STAT_C = 2.5


def stat_chunks(n):
    """misc.hip:349, 534: ceil(n / SD_STAT_CHUNK) chunks; (chunks, elements of the last)"""
    nc = -(-n // STAT_CHUNK)
    return nc, n - STAT_CHUNK * (nc - 1)


@dataclass(frozen=True)
class StatCase:
    n: int
    kind: str = "randn"  # randn: 3 z + 1 | offset: mean 100, spread 1

    @property
    def name(self):
        return f"n{self.n}-{self.kind}"


STAT_CASES = [StatCase(n) for n in STAT_NS] + [StatCase(4097, "offset")]
STAT = {c.name: c for c in STAT_CASES}


@functools.lru_cache(maxsize=None)
def stat_inputs(c):
    g = _g(5 + c.n)
    z = torch.randn(c.n, generator=g)
    return {"a": z * 3 + 1 if c.kind == "randn" else z + 100, "d": torch.randn(7, generator=g)}


def ref_stats(c, dt=F64, fault=None):
    """tools.tensorstats (oracle tensorstats, ref_cpu.py:595-597) of a; (mean - sub) / div and (std - sub) / div; and one
    slot of three requests: c + 0.5 mean(a) - 2 max(d). faults: "std_over_n"; "last_chunk_full" (the last chunk counted
    as SD_STAT_CHUNK elements: a zero-padded mean and std; min and max keep their guard)."""
    i = stat_inputs(c)
    a, d = i["a"].to(dt), i["d"].to(dt)
    src = a
    if fault == "last_chunk_full":
        src = F.pad(a, (0, STAT_CHUNK * stat_chunks(c.n)[0] - c.n))
    with sm.oracle_dtype(dt):
        ts = R.tensorstats(src, "a")
    mean, std = ts["a_mean"], ts["a_std"]
    if fault == "std_over_n":
        std = torch.std(src, unbiased=False)
    mn, mx = a.min(), a.max()
    am = a.abs().mean()
    out = {"mean": mean, "mean@scale": am, "min": mn.float(), "max": mx.float(),
           "affine": (mean - STAT_SUB) / STAT_DIV, "affine@scale": (am + STAT_SUB) / STAT_DIV,
           "combo": STAT_C + 0.5 * mean - 2.0 * d.max(), "combo@scale": STAT_C + 0.5 * am + 2.0 * d.max().abs()}
    if c.n > 1:
        # the deviations x - mean carry the rounding of x's own magnitude where the mean is far from 0
        out.update({"std": std, "std@scale": std, "affine_std": (std - STAT_SUB) / STAT_DIV,
                    "affine_std@scale": (std + STAT_SUB) / STAT_DIV})
    else:  # torch.std of one value is NaN; so is sqrt(0 / 0)
        out["nan"] = std.float()
    return {k: _np(torch.as_tensor(v).reshape(1)) for k, v in out.items()}


# =============================================================================================== loss terms
LT_BWD_FULL = 256 * 64  # misc.hip:557: nmax below it: ceil(nmax / 256) blocks; from it: 64 blocks, grid stride
LT_GT = 0.7


def loss_terms_gx(nmax):
    """misc.hip:557 sd_loss_terms_bwd"""
    return (nmax + 255) // 256 if nmax < LT_BWD_FULL else 64


@dataclass(frozen=True)
class LossTermsCase:
    ns: tuple

    @property
    def name(self):
        return "t" + "_".join(str(n) for n in self.ns)


LT_CASES = [LossTermsCase((255,)), LossTermsCase((1, 257, 16383)),
            LossTermsCase((1, 255, 257, 16383, 16384, 70000, 1, 257))]
LT = {c.name: c for c in LT_CASES}
LT_COEFS = (1.0, -1.0, 0.5, 1.0, 2.0, -0.25, 1.0, 3.0)
LT_SCALES = (0.5, 1.0, 2.0, 0.1, 1.5, 0.3, -0.7, 1.0)


@functools.lru_cache(maxsize=None)
def lt_inputs(c):
    g = _g(sum(c.ns))
    return {"xs": tuple(torch.randn(n, generator=g) + 0.3 for n in c.ns), "gm": torch.randn(len(c.ns), generator=g)}


def ordered_total_f32(means, scales):
    """misc.hip:383: tot = fadd(tot, fmul(scale_i, m_i)) in the dict's order, from 0, each operation rounded to float32"""
    tot = np.float32(0.0)
    for m, s in zip(np.asarray(means, np.float32), scales):
        tot = np.float32(tot + np.float32(np.float32(s) * m))
    return tot


def ref_loss_terms(c, dt=F64, fault=None):
    """dreamer.py:571-576: losses[k] = coef_k mean(x_k), total = sum(v * scale) over the dict in order (oracle
    ref_cpu.py:822), and the gradients of g_total total + sum g_means_i losses_i to every x.
    grads_<variant>: all = both upstream gradients, nogt = g_total null, nogm = g_means null.
    fault "scale_in_means": means_i = scale_i coef_i mean(x_i), the total their plain sum."""
    i = lt_inputs(c)
    k = len(c.ns)
    xs = [x.to(dt).requires_grad_() for x in i["xs"]]
    losses = {j: LT_COEFS[j] * xs[j].mean() for j in range(k)}
    if fault == "scale_in_means":
        losses = {j: v * LT_SCALES[j] for j, v in losses.items()}
        total = sum(v for v in losses.values())
    else:
        total = sum(v * LT_SCALES[j] for j, v in losses.items())
    means = torch.stack([losses[j] for j in range(k)])
    gm = i["gm"].to(dt)
    out = {"means": _np(means), "total": _np(total.reshape(1))}
    ms = np.array([abs(LT_COEFS[j]) * float(xs[j].detach().abs().mean()) for j in range(k)])
    out["means@scale"] = ms * (np.abs(LT_SCALES[:k]) if fault == "scale_in_means" else 1.0)
    out["total@scale"] = np.array([(ms * np.abs(LT_SCALES[:k])).sum()])
    for var, (gt, gmv) in {"all": (LT_GT, gm), "nogt": (0.0, gm), "nogm": (LT_GT, 0 * gm)}.items():
        gr = torch.autograd.grad(gt * total + (gmv * means).sum(), xs, retain_graph=True, allow_unused=True)
        gr = [g_ if g_ is not None else torch.zeros_like(x) for g_, x in zip(gr, xs)]
        out["grads_" + var] = np.concatenate([_np(g_) for g_ in gr])
        out["grads_" + var + "@scale"] = np.concatenate([
            np.full(n, (abs(gt * LT_SCALES[j]) + abs(float(gmv[j]))) * abs(LT_COEFS[j]) / n)
            for j, n in enumerate(c.ns)]) + 1e-30
    return out


# =============================================================================================== input preparation
PREP_NS = (1, 255, 257)
ONE_UP, ONE_DN = float(np.nextafter(np.float32(1), np.float32(2))), float(np.nextafter(np.float32(1), np.float32(0)))
SYMLOG_EDGES = (0.0, -0.0, 1e-30, -1e-30, 1e-8, -1e-8, 1.0, -1.0, 1e30, -1e30)
ACTION_EDGES = (0.0, -0.0, 0.5, -0.5, 1.0, -1.0, ONE_UP, -ONE_UP, ONE_DN, -ONE_DN, 7.0, -7.0)
MASK_BYTES = (0, 1, 255)
FLAG_BYTES = (0, 1, 2, 255)
U8_CP = ((1, 1), (1, 4), (3, 4), (4, 4), (3, 8))
U8_SHIFTS = (0.0, 0.5)


def _edged(n, edges, seed, scale):
    """n values: the edges first (as many as fit; with n = 1 the edge seed % len), then normal draws"""
    x = torch.randn(n, generator=_g(seed)) * scale
    e = torch.tensor(edges, dtype=F32)
    if n < len(e):
        e = e[seed % len(e):][:n]
    x[:len(e)] = e
    return x


@functools.lru_cache(maxsize=None)
def prep_inputs(n):
    g = _g(40 + n)
    d = {"symlog": _edged(n, SYMLOG_EDGES, 3 + n, 10.0), "action": _edged(n, ACTION_EDGES, 6 + n, 1.5),
         "last": torch.tensor(FLAG_BYTES, dtype=torch.uint8)[torch.randint(0, 4, (n,), generator=g)],
         "termb": torch.tensor(FLAG_BYTES, dtype=torch.uint8)[torch.randint(0, 4, (n,), generator=g)]}
    for w in (1, 7):
        for st in (1, 3):
            d[f"mx{w}"] = torch.randn(n, w, generator=g)
            mb = torch.tensor(MASK_BYTES, dtype=torch.uint8)[torch.randint(0, 3, (n * st,), generator=g)]
            mb[::st][:3] = torch.tensor(MASK_BYTES, dtype=torch.uint8)[:len(mb[::st][:3])]
            d[f"mask{w}s{st}"] = mb
    for C, _ in U8_CP:  # every byte value at every channel at least once where the pixels allow it
        d[f"img{C}"] = ((torch.arange(n * C) * 37 + 11 * n) % 256).to(torch.uint8).view(n, C)
    d["bytes"] = torch.arange(256, dtype=torch.uint8)
    return d


def _ulp_mag(q, y):
    return np.maximum(np.abs(_np(q)), np.abs(_np(y)))


def _u8(x, shift, dt):
    """dreamer.py:710-713 / networks.py:224: image / 255 (- 0.5), the quotient rounded to float32 once"""
    q = (x.to(dt) / 255.0)
    return q, q - shift


def ref_prep(n, dt=F64, fault=None):
    """symlog (oracle symlog, distributions.py:8-9); a / max(|a|, 1) (rssm.py:44); reset masking (rssm.py:161-165);
    episode flags; image / 255 - shift, channel-padded. `<name>_f32` is the float32 torch value the u8 kernels equal bit
    for bit (a correctly rounded division, then one subtraction); against float64 they are within 1 float32 ulp of the
    larger of quotient and result (v / 255 - 0.5 cancels near 0.5: the quotient's rounding is what remains)."""
    i = prep_inputs(n)
    out = {}
    x = i["symlog"].to(dt)
    with sm.oracle_dtype(dt):
        out["symlog"] = _np(R.symlog(x))
    out["symlog@scale"] = np.abs(_np(R.symlog(i["symlog"].double()))) + 1e-45
    a = i["action"].to(dt)
    out["action_norm"] = _np(a / torch.clip(torch.abs(a), min=1.0))
    for w in (1, 7):
        for st in (1, 3):
            keep = (i[f"mask{w}s{st}"][::st] == 0)[:, None]
            out[f"mask_rows_w{w}s{st}"] = _np(torch.where(keep, i[f"mx{w}"], torch.zeros(())))
    la, te = (i["last"] != 0).float(), (i["termb"] != 0).float()
    out.update(last=_np(la), term=_np(te), cont=_np(1.0 - te))
    for sh in U8_SHIFTS:
        tag = f"s{sh:g}"
        q, y = _u8(i["bytes"], sh, dt)
        q32, y32 = _u8(i["bytes"], sh, F32)
        out[f"u8_{tag}"], out[f"u8_{tag}@mag"], out[f"u8_f32_{tag}"] = _np(y), _ulp_mag(q, y), _np(y32)
        for C, Cp in U8_CP:
            q, y = _u8(i[f"img{C}"], sh, dt)
            q32, y32 = _u8(i[f"img{C}"], sh, F32)
            key = f"c{C}p{Cp}{tag}"
            padz = (0, Cp - C)
            out[f"enc_{key}"], out[f"enc_{key}@mag"] = _np(F.pad(y, padz)), _ulp_mag(F.pad(q, padz), F.pad(y, padz))
            out[f"enc_f32_{key}"] = _np(F.pad(y32, padz))
            if sh == 0.0:
                out[f"img_{key}"], out[f"img_{key}@mag"], out[f"img_f32_{key}"] = _np(q), _ulp_mag(q, q), _np(q32)
            # sd_pad_channels: float input x - shift, padded: x = the float32 quotient
            yp = q32.to(dt) - sh
            out[f"pad_{key}"], out[f"pad_{key}@mag"] = _np(F.pad(yp, padz)), _ulp_mag(F.pad(q32, padz), F.pad(yp, padz))
            out[f"pad_f32_{key}"] = _np(F.pad(q32 - sh, padz))
    return out


# =============================================================================================== optimiser
CHUNK = 16384  # optim.py:19
OPT_SIZES = (1, 3, 63, 64, 65, 16383, 16384, 16385, 3 * 16384 + 5, 257 * 16384 + 2)
OPT_PSCALE = (1.0, 0.0, 1.0, 0.0, 100.0, 1.0, 100.0, 1.0, 1.0, 100.0)  # 0: an all-zero parameter (bias, norm-adjacent)
OPT_ZERO_GRAD = 2  # this tensor's gradient is all zero
OPT_GATED = 6
OPT_STEPS = 3
OPT_GSTEP = (0.01, 10.0, 0.01)  # step 2's gradients are 1000 x larger
OPT_HP = dict(lr=4e-5, betas=(0.9, 0.999), eps=1e-20, agc=0.3, pmin=1e-3)
AGC_MARGIN = 1e-3


def arena_layout(sizes):
    """optim.py:34-39, 47-53 FlatArena in the identity order: (offsets, total, chunk_beg, chunk_end, chunk_tensor,
    tensor_chunk0)"""
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off += (n + 63) // 64 * 64
    beg, end, tens, t0 = [], [], [], [0]
    for ti, (o, n) in enumerate(zip(offs, sizes)):
        for c in range(0, max(n, 1), CHUNK):
            beg.append(o + c)
            end.append(o + min(n, c + CHUNK))
            tens.append(ti)
        t0.append(len(beg))
    return offs, off, beg, end, tens, t0


def chunked_norm(x):
    """optim.hip:41-48, 64-67: sqrt of the sum of the tensor's per-chunk sums of squares (the oracle's float32
    torch norm of 4 M elements alone is 1e-4 off: its accumulation, not the operation)"""
    x = x.reshape(-1)
    return torch.sqrt(torch.stack([(x[lo:lo + CHUNK] * x[lo:lo + CHUNK]).sum()
                                   for lo in range(0, max(x.numel(), 1), CHUNK)]).sum())


def chunk_sum_strides(nchunks_of_tensor):
    """optim.hip:64: a tensor's chunk sums over 256 threads"""
    return -(-nchunks_of_tensor // 256)


@dataclass(frozen=True)
class OptCase:
    warmup: int
    variant: str = "plain"  # plain | gs (grad_scale 1/4) | gate0 | gate1 | zg (zero_grads)

    @property
    def name(self):
        return f"w{self.warmup}-{self.variant}"

    @property
    def grad_scale(self):
        return 0.25 if self.variant == "gs" else 1.0

    @property
    def gate(self):
        return {"gate0": 0.0, "gate1": 1.0}.get(self.variant)


OPT_CASES = [OptCase(0), OptCase(1000)] + [OptCase(1000, v) for v in ("gs", "gate0", "gate1", "zg")]
OPT = {c.name: c for c in OPT_CASES}


@functools.lru_cache(maxsize=None)
def opt_inputs():
    g = _g(0)
    ps = tuple(torch.randn(n, generator=g) * s for n, s in zip(OPT_SIZES, OPT_PSCALE))
    grads = tuple(tuple(torch.zeros(n) if j == OPT_ZERO_GRAD else torch.randn(n, generator=g) * OPT_GSTEP[it]
                        for j, n in enumerate(OPT_SIZES)) for it in range(OPT_STEPS))
    return {"p": ps, "g": grads}


def _oracle_agent(ps, warmup):
    ag = R.OracleAgent.__new__(R.OracleAgent)
    ag.P = {str(j): p.clone().requires_grad_() for j, p in enumerate(ps)}
    ag.s = types.SimpleNamespace(shapes={str(j): tuple(p.shape) for j, p in enumerate(ps)})
    ag.lr0, ag.warmup, ag.betas, ag.eps = OPT_HP["lr"], warmup, OPT_HP["betas"], OPT_HP["eps"]
    ag.agc, ag.pmin = OPT_HP["agc"], OPT_HP["pmin"]
    ag.opt_step, ag.state = 0, {}
    return ag


def _agc_restated(ag, fault):
    """OracleAgent.agc_ (agc.py:15-53) with a fault planted: "agc_no_pmin"; "clip_from_chunk" (each chunk of CHUNK
    elements clipped by its own norms)"""
    with torch.no_grad():
        for p in ag.trainable():
            g = p.grad
            for lo in range(0, max(p.numel(), 1), CHUNK if fault == "clip_from_chunk" else max(p.numel(), 1)):
                hi = lo + (CHUNK if fault == "clip_from_chunk" else p.numel())
                pn, gn = torch.linalg.vector_norm(p.data[lo:hi]), torch.linalg.vector_norm(g[lo:hi])
                upper = (pn if fault == "agc_no_pmin" else torch.clamp(pn, min=ag.pmin)) * ag.agc
                g[lo:hi] *= 1.0 / torch.clamp(gn / upper, min=1.0)


def _laprop_restated(ag, fault):
    """OracleAgent.laprop_step (laprop.py:46-118) with "bc1_not_over_lr" planted: bias correction lr_ema1, not
    lr_ema1 / lr"""
    lr = ag.lr()
    b1, b2 = ag.betas
    with torch.no_grad():
        for p in ag.trainable():
            g = p.grad.data
            st = ag.state.get(id(p))
            if st is None:
                st = ag.state[id(p)] = dict(step=0, exp_avg=torch.zeros_like(p.data), exp_avg_lr_1=0.0,
                                            exp_avg_lr_2=0.0, exp_avg_sq=torch.zeros_like(p.data))
            st["step"] += 1
            st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1 - b2)
            st["exp_avg_lr_1"] = st["exp_avg_lr_1"] * b1 + (1 - b1) * lr
            st["exp_avg_lr_2"] = st["exp_avg_lr_2"] * b2 + (1 - b2)
            bc1 = st["exp_avg_lr_1"] if fault == "bc1_not_over_lr" else (st["exp_avg_lr_1"] / lr if lr != 0.0 else 1.0)
            denom = st["exp_avg_sq"].div(st["exp_avg_lr_2"]).sqrt_().add_(ag.eps)
            st["exp_avg"].mul_(b1).add_(g / denom, alpha=(1 - b1) * lr)
            p.data.add_(st["exp_avg"], alpha=-(1 / bc1))


def ref_optim(c, dt=F64, fault=None, restated=False, scales=True):
    """Three steps of clip_grad_agc_ -> LaProp.step -> scheduler.step through the oracle's own agc_ / laprop_step / lr
    (gradients times grad_scale and the gate first: the data-parallel mean, DreamerPro's prototype freeze). Per step:
    the parameter deltas, both moments, the pre-clip gradient norms (float64 of the inputs), the scalar state (step,
    lr_ema1, lr_ema2, lr) and the AGC ratios. Faults ride on a restated copy (`restated` runs it without one, to be
    compared with the oracle bit for bit): "agc_no_pmin", "clip_from_chunk", "bc1_not_over_lr", "gate_after_norm",
    "step_not_advanced" (the scheduler's count: only warm-up 1000 shows it). scales = False leaves the Σ|terms| out (a
    restatement's own are never read)."""
    i = opt_inputs()
    ag = _oracle_agent([p.to(dt) for p in i["p"]], c.warmup)
    use_copy = restated or fault is not None
    b1 = OPT_HP["betas"][0]
    seg, lo = [], 0
    for n in OPT_SIZES:
        seg.append((lo, lo + n))
        lo += n
    out = {"@seg": seg}
    cat = lambda ts: np.concatenate([_np(t).reshape(-1) for t in ts])  # noqa: E731
    m_scale = [torch.zeros(n, dtype=F64) for n in OPT_SIZES]
    for it in range(OPT_STEPS):
        ps = ag.trainable()
        gn, ratio = [], []
        for j, p in enumerate(ps):
            gs = c.grad_scale * (c.gate if (c.gate is not None and j == OPT_GATED) else 1.0)
            g = i["g"][it][j].to(dt)
            if fault == "gate_after_norm" and j == OPT_GATED and c.gate is not None:
                p.grad = g * c.grad_scale  # the norms below see the ungated gradient
            else:
                p.grad = g * gs
            g64 = i["g"][it][j].double() * gs
            gn.append(chunked_norm(p.grad if fault == "gate_after_norm" else g64.to(dt)).double())
            pn64 = torch.linalg.vector_norm(p.data.double())
            ratio.append(float(torch.linalg.vector_norm(g64) / (max(float(pn64), OPT_HP["pmin"]) * OPT_HP["agc"])))
        prev = [p.data.clone() for p in ps]
        if use_copy:
            _agc_restated(ag, fault)
            if fault == "gate_after_norm" and c.gate is not None:
                ps[OPT_GATED].grad *= c.gate
        else:
            ag.agc_()
        gclip = [p.grad.double().clone() for p in ps]
        lr = ag.lr()
        (_laprop_restated(ag, fault) if use_copy else ag.laprop_step())
        if fault != "step_not_advanced":
            ag.opt_step += 1
        sts = [ag.state[id(p)] for p in ps]
        s0 = sts[0]
        k = str(it)
        out["dp" + k] = cat([p.data.double() - q.double() for p, q in zip(ps, prev)])
        out["m" + k] = cat([st["exp_avg"] for st in sts])
        out["v" + k] = cat([st["exp_avg_sq"] for st in sts])
        out["gn" + k] = np.array([float(x) for x in gn])
        out["scalars" + k] = np.array([float(s0["step"]), s0["exp_avg_lr_1"], s0["exp_avg_lr_2"], lr], np.float64)
        out["@ratio" + k] = np.array(ratio)
        if not scales:
            continue
        bc1 = s0["exp_avg_lr_1"] / lr
        # Σ|terms| of exp_avg: b1 * (the previous step's) + |a1 g / denom|, carried from step to step
        for j, st in enumerate(sts):
            denom = st["exp_avg_sq"].double().div(s0["exp_avg_lr_2"]).sqrt() + OPT_HP["eps"]
            m_scale[j] = b1 * m_scale[j] + (1 - b1) * lr * (gclip[j].abs() / denom)
        out["dp" + k + "@scale"] = (cat([s / bc1 for s in m_scale]) + 1e-300).astype(np.float32)
        # the update's own addition rounds p once: half an ulp of the larger of p before and after
        pm = cat([torch.maximum(p.data.double().abs(), q.double().abs()) for p, q in zip(ps, prev)])
        out["dp" + k + "@floor"] = (0.5 * parity.ulp(pm * (1 + 1e-6))).astype(np.float32)  # of p's binade, or the next
        out["dp" + k + "@ulp"] = parity.ulp(cat([p.data for p in ps])).astype(np.float32)
        out["m" + k + "@scale"] = (cat(m_scale) + 1e-300).astype(np.float32)
        out["v" + k + "@scale"] = np.abs(out["v" + k]).astype(np.float32)
        out["gn" + k + "@scale"] = out["gn" + k] + 1e-300
    return out


POLYAK_NS = (1, 255, 257, 100003)
POLYAK_MIX = (0.02, 1.0)


@functools.lru_cache(maxsize=None)
def polyak_inputs(n):
    g = _g(3 + n)
    return {"src": torch.randn(n, generator=g), "dst": torch.randn(n, generator=g)}


def ref_polyak(case, dt=F64, fault=None):
    """dreamer.py:242-249 through the oracle's update_slow_target: slow = mix * value + (1 - mix) * slow"""
    n, mix = case
    i = polyak_inputs(n)
    ag = R.OracleAgent.__new__(R.OracleAgent)
    ag.P = {"v": i["src"].to(dt), "s": i["dst"].to(dt).clone()}
    ag.s = types.SimpleNamespace(slow_names={"v": "s"},
                                 cfg=types.SimpleNamespace(slow_target_fraction=mix, slow_target_update=1))
    ag.slow_updates = 0
    ag.update_slow_target()
    sc = (mix * i["src"].double()).abs() + ((1 - mix) * i["dst"].double()).abs()
    return {"dst": _np(ag.P["s"]), "dst@scale": _np(sc) + 1e-300}


POLYAK_CASES = [(n, m) for n in POLYAK_NS for m in POLYAK_MIX]


# =============================================================================================== replay slices
SL_CAP, SL_E, SL_L = 7, 2, 3
SL_STARTS = ((5, 0), (6, 1), (2, 0), (3, 0), (4, 0), (0, 1))  # (t0, env): 5 and 6 wrap around cap
SL_PICK = (0, 1, 2, 3, 4, 5, 2)  # slices 2, 3, 4 overlap on env 0; slice 6 repeats slice 2
# key: (name, dtype, row elements, steps, shift, base offset in elements of the key's dtype)
SL_KEYS = (("vec16", "float32", 4, SL_L, 1, 0), ("b1", "uint8", 1, SL_L, 1, 0), ("b12", "float32", 3, SL_L, 1, 0),
           ("b20", "float32", 5, SL_L, 1, 0), ("mis16", "float32", 4, SL_L, 1, 1),
           ("initial", "float32", 4, 1, 0, 0), ("action", "float32", 4, SL_L, 0, 0))
SL_ACTION = "action"
SL_SENT = 77.0


def slice_path(row_bytes, src_off, dst_off):
    """misc.hip:807: 16-byte copies when the row is a multiple of 16 bytes and both rows start 16-byte aligned (the
    offsets are from a 16-byte aligned allocation), bytes otherwise"""
    return "vector" if row_bytes % 16 == 0 and (src_off | dst_off) % 16 == 0 else "bytes"


def slice_key_paths(key):
    """the set of copy paths a key's rows take in the gather"""
    _, dtype, w, steps, _, base = key
    es = np.dtype(dtype).itemsize
    rb = w * es
    return {slice_path(rb, base * es + (t * SL_E + e) * rb, (b * steps + j) * rb)
            for t in range(SL_CAP) for e in range(SL_E) for b in range(len(SL_PICK)) for j in range(steps)}


@functools.lru_cache(maxsize=None)
def slice_storage():
    """{key: (cap, E, w) array}: every element distinct"""
    out = {}
    for k, (name, dtype, w, _, _, _) in enumerate(SL_KEYS):
        v = np.arange(SL_CAP * SL_E * w).reshape(SL_CAP, SL_E, w) + 1000 * k
        out[name] = (v % 251 if dtype == "uint8" else v).astype(dtype)
    return out


def ref_slices_gather(fault=None):
    """utils/buffer.py:27-42: slice b starts at (t0, e) = starts[pick[b]]; a key's step j is storage row
    ((t0 + shift + j) % cap, e); the write-back index is the data rows' (shift 1). fault "action_shift_1"."""
    st = slice_storage()
    B = len(SL_PICK)
    out = {"t_idx": np.zeros((B, SL_L), np.int64), "e_idx": np.zeros((B, SL_L), np.int64)}
    for name, dtype, w, steps, shift, _ in SL_KEYS:
        if fault == "action_shift_1" and name == SL_ACTION:
            shift = 1
        o = np.zeros((B, steps, w), dtype)
        for b, pk in enumerate(SL_PICK):
            t0, e = SL_STARTS[pk]
            for j in range(steps):
                o[b, j] = st[name][(t0 + shift + j) % SL_CAP, e]
        out[name] = o
    for b, pk in enumerate(SL_PICK):
        t0, e = SL_STARTS[pk]
        for j in range(SL_L):
            out["t_idx"][b, j], out["e_idx"][b, j] = (t0 + 1 + j) % SL_CAP, e
    return out


def slice_scatter_batch(w):
    """(B, L, w) values to write back: every element distinct and none the sentinel"""
    B = len(SL_PICK)
    return (np.arange(B * SL_L * w).reshape(B, SL_L, w) + 100.0).astype(np.float32)


def ref_slices_scatter(w, fault=None):
    """utils/buffer.py:44-53 with the overlap rule of misc.hip:791-796: rows written in slice order, so the largest b
    wins; every row no slice covers keeps the sentinel. -> (storage (cap, E, w), writers per row (cap, E)).
    fault "smallest_b_wins"."""
    sto = np.full((SL_CAP, SL_E, w), SL_SENT, np.float32)
    cnt = np.zeros((SL_CAP, SL_E), np.int64)
    bat = slice_scatter_batch(w)
    order = range(len(SL_PICK))
    for b in (reversed(order) if fault == "smallest_b_wins" else order):
        t0, e = SL_STARTS[SL_PICK[b]]
        for j in range(SL_L):
            sto[(t0 + 1 + j) % SL_CAP, e] = bat[b, j]
            cnt[(t0 + 1 + j) % SL_CAP, e] += 1
    return sto, cnt


# =============================================================================================== registry
FAMILIES = {
    "barlow": (BARLOW_CASES, ref_barlow),
    "infonce": (NCE_CASES, ref_infonce),
    "stats": (STAT_CASES, ref_stats),
    "loss_terms": (LT_CASES, ref_loss_terms),
    "prep": (PREP_NS, ref_prep),
    "optim": (OPT_CASES, ref_optim),
    "polyak": (POLYAK_CASES, ref_polyak),
}
FAULTS = {
    "barlow": ("biased_std", "mean_padded_ld", "drop_last_partial", "lambda_on_diag", "no_mean_dn", "shard_R_for_Nt"),
    "infonce": ("no_rowmax", "label_at_r", "mean_256_rows"),
    "stats": ("std_over_n", "last_chunk_full"),
    "loss_terms": ("scale_in_means",),
    "optim": ("agc_no_pmin", "clip_from_chunk", "bc1_not_over_lr", "gate_after_norm", "step_not_advanced"),
}
# A fault that, where it changes bits without failing, is a correct float32 evaluation and not an error: the sum of
# exp without the row maximum is exact arithmetic's log-sum-exp until exp overflows float32, so it must fail from
# there on (mag 100) and may pass below (mag 0, 80).
FAULT_VALID_BELOW = {"no_rowmax": lambda c: c.mag < EXP_OVERFLOW_F32}


def case_name(case):
    if isinstance(case, int):
        return str(case)
    return getattr(case, "name", None) or "-".join(str(x) for x in case)


@functools.lru_cache(maxsize=None)
def _reference(fam, case):
    return FAMILIES[fam][1](case)


def reference(fam, case):
    """the float64 reference, computed once and shared (the optimiser's is 0.5 GB a case: computed where it is used)"""
    return FAMILIES[fam][1](case) if fam == "optim" else _reference(fam, case)
