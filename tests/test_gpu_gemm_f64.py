"""The dense contractions (csrc/gemm.hip, csrc/gemm3.hip) against float64 at every arm of their dispatch: the case
tables, guarded inputs, references and bounds of tests/gemm_models.py. Every launch runs inside
sentinel-filled allocations: C's padding, the neighbouring batch entries' rows, the band behind part_out and the
workspace past the contract's size are compared bit for bit after it. Launches go through sdreamer.kernels (gemm,
wgrad, wgrad2, mlp_layer); the C ABI directly only where it alone admits the arm (an explicit workspace size, K = 0,
accumulate = 0, null per-entry pointers beside set ones, the split-bf16 entry's own f32 route, refusals)."""
import ctypes
from dataclasses import replace

import numpy as np
import pytest
import torch

import gemm_models as gm

pytestmark = pytest.mark.gpu

ENTRY = {"f32": "sd_gemm_f32", "bf16x3": "sd_gemm_bf16x3", "wgrad": "sd_gemm_bf16x3_wgrad",
         "wgrad2": "sd_gemm_bf16x3_wgrad2", "mlp": "sd_gemm_bf16x3_mlp"}


class Dev:
    """a Buf's allocation on the device"""

    def __init__(self, buf):
        self.buf = buf
        self.flat = buf.host.cuda() if buf is not None else None

    @property
    def view(self):
        return self.buf.view(self.flat)

    @property
    def ptr(self):
        return 0 if self.buf is None else self.flat.data_ptr() + 4 * self.buf.start

    def host_view(self):
        return self.buf.view(self.flat.cpu()).to(torch.float64).numpy()

    def problems(self, what, output=False):
        """input: nothing in the allocation changed; output: nothing outside the view"""
        if self.buf is None:
            return []
        bad = self.buf.changed_outside(self.flat, None if output else torch.zeros(self.buf.n, dtype=torch.bool))
        return [f"{what}: {len(bad)} floats changed outside what the launch may write, first at {bad[0]} "
                f"(view {self.buf.start}..{self.buf.start + self.buf.ext})"] if bad else []


def _sq(t, batch):
    return t[0] if batch == 1 else t


def gemm_desc(nat, c, inp, dv):
    d, n = nat.GemmDesc(), inp.d
    d.A, d.B, d.C, d.bias = dv["A"].ptr, dv["B"].ptr, dv["C"].ptr, (dv["bias"].ptr or None)
    d.lda, d.ldb, d.ldc = n.lda, n.ldb, n.ldc
    d.strideA, d.strideB, d.strideC, d.strideBias = n.sA, n.sB, n.sC, n.sBias
    d.M, d.N, d.K, d.batch = c.M, c.N, c.K, c.batch
    d.a_kcontig, d.b_kcontig, d.ksplit, d.tile = int(c.ak), int(c.bk), c.ksplit, c.tile
    d.alpha, d.beta = c.alpha, c.beta
    return d


def gemm_args(nat, K, c, d, dv, ws_floats=None):
    ws = dv["ws"]
    n = ws.buf.ext if ws_floats is None else ws_floats
    args = [ctypes.byref(d), ws.ptr if ws.buf.ext else 0, n]
    if c.entry == "wgrad":
        args += [dv["rs"].ptr, c.acc]
    elif c.entry == "wgrad2":
        args += [dv["rs"].ptr, dv["rs2"].ptr, c.rs_split, c.acc]
    return args + [K.stream()]


def _gemm_dev(inp):
    return {"A": Dev(inp.bufA), "B": Dev(inp.bufB), "C": Dev(inp.bufC), "bias": Dev(inp.bufBias), "rs": Dev(inp.bufRs),
            "rs2": Dev(inp.bufRs2), "ws": Dev(inp.bufWs)}


def _guards(dv):
    bad = []
    for k, v in dv.items():
        bad += v.problems(k, output=k in ("C", "rs", "rs2", "ws"))
    return bad


def run_gemm(c):
    """launch case c; ({output: float64 ndarray}, [guard problems])"""
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    inp = gm.gemm_inputs(c)
    dv = _gemm_dev(inp)
    wg = c.entry.startswith("wgrad")
    if c.abi:
        d = gemm_desc(nat, c, inp, dv)
        nat.call(ENTRY[c.entry], *gemm_args(nat, K, c, d, dv))
    else:
        a, b, out = _sq(dv["A"].view, c.batch), _sq(dv["B"].view.transpose(1, 2), c.batch), _sq(dv["C"].view, c.batch)
        bias = None if not c.bias else dv["bias"].view if c.bias == 2 else dv["bias"].view[0]
        if c.group == "wgrad-py":
            if c.entry == "wgrad":
                K.wgrad(a.t(), b, out, dv["rs"].view)
            else:
                assert K.wgrad2(a.t(), b, out, dv["rs"].view, dv["rs2"].view, c.rs_split)
        elif wg:
            assert c.entry == "wgrad" and c.acc == 1
            ok = K.gemm(a, b, out, alpha=c.alpha, beta=c.beta, ksplit=c.ksplit, tile=c.tile, fast=True,
                        rowsum=dv["rs"].view)
            assert ok is not False
        else:
            K.gemm(a, b, out, bias=bias, alpha=c.alpha, beta=c.beta, ksplit=c.ksplit, tile=c.tile,
                   fast=c.entry == "bf16x3")
    torch.cuda.synchronize()
    got = {"C": dv["C"].host_view()}
    if wg:
        got["rowsum"] = dv["rs"].host_view()
        if c.entry == "wgrad2":
            got["rowsum2"] = dv["rs2"].host_view()
    return got, _guards(dv)


# ------------------------------------------------------------------------------------------------ the MLP entry
def _mlp_dev(inp):
    dv = {"x": Dev(inp.bufX), "C": Dev(inp.bufC), "pin": Dev(inp.bufPin), "pout": Dev(inp.bufPout)}
    for k, bufs in (("w", inp.bufW), ("bias", inp.bufBias), ("nw", inp.bufNw)):
        for i, b in enumerate(bufs):
            dv[f"{k}{i}"] = Dev(b)
    return dv


def mlp_abi(nat, K, c, dv):
    """the descriptor and extension of case c as kernels.mlp_layer builds them; the per-entry form with entry c.null's
    pointers null, served by the strided operands (B, bias, norm_w with stride 0 at that entry's tensors)"""
    d, e = nat.GemmDesc(), nat.MlpExt()
    d.A, d.C = dv["x"].ptr, dv["C"].ptr
    d.lda, d.ldb, d.ldc = dv["x"].buf.strides[1], c.K, c.N
    d.strideA, d.strideC = dv["x"].buf.strides[0], c.M * c.N
    d.M, d.N, d.K, d.batch = c.M, c.N, c.K, c.batch
    d.a_kcontig, d.b_kcontig, d.ksplit, d.tile = 1, 1, 1, 0
    d.alpha, d.beta = c.alpha, 0.0
    if c.rows:
        z = max(c.null, 0)
        d.B, d.bias, d.strideB, d.strideBias = dv[f"w{z}"].ptr, (dv[f"bias{z}"].ptr if c.null >= 0 else None), 0, 0
        for b in range(c.batch):
            if b == c.null:
                continue
            e.w_ptr[b], e.bias_ptr[b] = dv[f"w{b}"].ptr, dv[f"bias{b}"].ptr
            e.w_rows[b] = c.rows[b] if c.rows[b] < c.N else 0
            if c.rms:
                e.norm_w_ptr[b] = dv[f"nw{b}"].ptr
        if c.rms and c.null >= 0:
            e.norm_w, e.stride_norm_w = dv[f"nw{c.null}"].ptr, 0
    else:
        d.B, d.bias, d.strideB, d.strideBias = dv["w0"].ptr, dv["bias0"].ptr, c.N * c.K, c.N
        if c.rms:
            e.norm_w, e.stride_norm_w = dv["nw0"].ptr, c.K
    if c.rms:
        e.part_in, e.stride_part_in, e.npart_in = dv["pin"].ptr, c.npin * c.M, c.npin
        e.act, e.eps = c.act, K.EPS
    if c.pout:
        e.part_out, e.stride_part_out = dv["pout"].ptr, (c.N // 64) * c.M
    return d, e


def run_mlp(c):
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    inp = gm.mlp_inputs(c)
    dv = _mlp_dev(inp)
    if c.null >= 0:
        d, e = mlp_abi(nat, K, c, dv)
        nat.call(ENTRY["mlp"], ctypes.byref(d), ctypes.byref(e), K.stream())
    else:
        n = c.batch
        if c.rows:
            w, bias = [dv[f"w{b}"].view for b in range(n)], [dv[f"bias{b}"].view for b in range(n)]
            nw = [dv[f"nw{b}"].view for b in range(n)] if c.rms else None
        else:
            w, bias, nw = dv["w0"].view, dv["bias0"].view, dv["nw0"].view if c.rms else None
        ok = K.mlp_layer(dv["x"].view, w, dv["C"].view, bias=bias, norm_w=nw, part_in=dv["pin"].view if c.rms else None,
                         part_out=dv["pout"].view if c.pout else None, act=c.act, alpha=c.alpha)
        assert ok, "the fused MLP entry refused the case"
    torch.cuda.synchronize()
    got = {"C": dv["C"].host_view()}
    if c.pout:
        got["pout"] = dv["pout"].host_view()
        got["pout_own"] = gm.own_pout(got["C"])
    bad = []
    for k, v in dv.items():
        bad += v.problems(k, output=k in ("C", "pout"))
    return got, bad, (inp, dv)


def run(c):
    return run_mlp(c)[:2] if isinstance(c, gm.Mlp) else run_gemm(c)


# ------------------------------------------------------------------------------------------------ the comparison
WORST = {}


def check(c):
    fam = gm.family(c)
    inp = gm.inputs(c)
    ref = gm.evaluate(c, inp)
    arm = None if fam == "mlp" else gm.arm_of(c, inp.d)
    fam_c = "f32" if gm.routed_f32(c, arm) else fam
    split = gm.evaluate(c, inp, "split", gm.F64) if fam_c != "f32" else None
    got, bad = run(c)
    bad = bad + gm.failures(fam, got, ref, split, arm)
    for k, v in gm.units(fam_c, got, ref, split).items():
        key = (fam if fam_c == fam else fam + "->f32", k)
        WORST[key] = max(WORST.get(key, (0.0, "")), (v, c.name))
    return [f"{c.name}: {b}" for b in bad]


def _groups(fam):
    seen = []
    for c in gm.CASES[fam]:
        if c.group not in seen:
            seen.append(c.group)
    return [(fam, g) for g in seen]


@pytest.mark.parametrize("fam,group", [fg for fam in gm.CASES for fg in _groups(fam)])
def test_against_float64(fam, group):
    """every case of the group: outputs inside their elementwise bounds and caps, guard bands intact"""
    bad = []
    cases = [c for c in gm.CASES[fam] if c.group == group]
    for c in cases:
        bad += check(c)
    print(f"{fam}/{group}: {len(cases)} cases; worst so far (units, case):",
          {f"{f}.{k}": (round(v, 3), n) for (f, k), (v, n) in WORST.items() if f.startswith(fam)})
    assert not bad, "\n".join(bad[:20])


def test_fallback_is_the_f32_route():
    """M, N or K = 63 on sd_gemm_bf16x3: at the f32 tolerance (a split-bf16 product would miss it a hundredfold)"""
    for c in (c for c in gm.G3_CASES if c.group == "fallback"):
        inp = gm.inputs(c)
        assert gm.arm_of(c, inp.d).fallback
        got, bad = run_gemm(c)
        ref = gm.evaluate(c, inp)
        assert not bad and not gm.failures("f32", got, ref, None)
        sp = gm.evaluate(c, inp, "split", gm.F32)
        assert gm.failures("f32", sp, ref, None), "the split model itself passes the f32 bound: the case shows nothing"


@pytest.mark.parametrize("N", [64, 192, 320])
@pytest.mark.parametrize("form", ["strided", "entries"])
def test_part_out_at_odd_64s_feeds_the_next_layer(N, form):
    """N = 64 * odd with part_out, batch 3: the last column tile's second half lies past N. Every entry's partials
    (the last entry's too) against float64, the band behind part_out untouched, and a second mlp_layer normalised by
    those partials against its float64 reference (a zeroed partial 0 of entry b + 1 gives rstd = 1 / sqrt(eps))."""
    from sdreamer import kernels as K
    c = gm.Mlp(129, N, 32, batch=3, rms=True, pout=True, npin=3, rows=(N, N, N) if form == "entries" else ())
    inp0 = gm.inputs(c)
    ref, split = gm.evaluate(c, inp0), gm.evaluate(c, inp0, "split", gm.F64)
    got, bad, (inp, dv) = run_mlp(c)
    bad = bad + gm.failures("mlp", got, ref, split)
    assert not bad, "\n".join(bad)
    # the second layer: x = this launch's C, part_in = this launch's part_out, on the device as they are
    c2 = gm.Mlp(129, 64, N, batch=3, rms=True, npin=N // 64)
    in2 = gm.mlp_inputs(c2)
    in2.x = torch.from_numpy(got["C"]).float()
    in2.pin = torch.from_numpy(got["pout"]).float()
    w, b, nw = (torch.stack(in2.W).cuda(), torch.stack(in2.bias).cuda(), in2.nw.cuda())
    out = torch.empty(3, 129, 64, device="cuda")
    assert K.mlp_layer(dv["C"].view, w, out, bias=b, norm_w=nw, part_in=dv["pout"].view)
    got2 = {"C": out.double().cpu().numpy()}
    bad = gm.failures("mlp", got2, gm.evaluate(c2, in2), gm.evaluate(c2, in2, "split", gm.F64))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ refusals
def _apply_dim(d, key, val):
    setattr(d, key, val)


@pytest.mark.parametrize("name", [r.name for r in gm.REFUSALS])
def test_refusal(name):
    """each SD_EARG / SD_ESHAPE line of the four entry points (and the empty problems' SD_OK): the code, and nothing
    in any guarded buffer changed: refused before any launch"""
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    r = next(r for r in gm.REFUSALS if r.name == name)
    c, (what, val) = r.base, r.change
    if r.entry == "mlp":
        inp = gm.mlp_inputs(c)
        dv = _mlp_dev(inp)
        d, e = mlp_abi(nat, K, c, dv)
        xp = ctypes.byref(e)
        if what == "null":
            if val == "x":
                xp = None
            else:
                setattr(d, val, None)
        elif what == "dim":
            _apply_dim(d, *val)
        elif what == "ext":
            setattr(e, val[0], val[1])
        elif what == "ext_entry":
            f, b, v = val
            getattr(e, f)[b] = (getattr(e, f)[b] + 4) if v == "+1" else v
        rc = nat.fns[ENTRY["mlp"]](ctypes.byref(d), xp, K.stream())
    else:
        inp = gm.gemm_inputs(c)
        dv = _gemm_dev(inp)
        d = gemm_desc(nat, c, inp, dv)
        ws_floats = None
        if what == "null" and val in ("A", "B", "C"):
            setattr(d, val, None)
        elif what == "tile":
            d.tile = val
        elif what == "dim":
            _apply_dim(d, *val)
        elif what == "ws" and val is not None:
            ws_floats = dv["ws"].buf.ext + val
        if what == "rs_split":
            c = replace(c, rs_split=val)
        args = gemm_args(nat, K, c, d, dv, ws_floats)
        if what == "ws" and val is None:
            args[1] = 0
        if what == "null" and val == "rowsum":
            args[3] = 0
        if what == "null" and val == "rowsum2":
            args[4] = 0
        rc = nat.fns[ENTRY[r.entry]](*args)
    torch.cuda.synchronize()
    assert rc == r.expect, (name, rc, r.expect)
    bad = []
    for k, v in dv.items():
        bad += v.problems(k)
    assert not bad, "\n".join(bad)


def test_zz_report_worst():
    """the measured column of DESIGN.md § 2.5: the worst distance per family and output, in the output's own unit"""
    for (fam, k), (v, n) in sorted(WORST.items()):
        print(f"MEASURED {fam} {k}: {v:.3f} units at {n}")
        tol = gm.TOL[fam.split("->")[-1] if "->" in fam else fam][k if k != "rowsum2" else "rowsum"]
        assert v <= tol.k
    assert np.isfinite([v for v, _ in WORST.values()]).all()
