"""The small row kernels — csrc/rownorm.hip (RMSNorm + SiLU, column sums), csrc/dist.hip (sampler, discrete and bounded
normal actor heads, KL, two-hot, replay-value and actor-critic losses, Bernoulli, GRU gates) and csrc/returns.hip
(λ-return, ReturnEMA) — against float64 at the smallest shapes that reach every arm of their dispatch
(tests/rowop_models.py holds the tables, inputs, references and comparison; tests/test_rowop_parity_cpu.py checks on
the CPU that the tables reach the arms, that the float32 restatement passes with room and that planted faults fail;
DESIGN.md § 2.3 lists the cases with the arm each reaches and the measured figures).

Every output is compared elementwise (parity.assert_close, atol = tol * max(|ref_i|, 1), or a stated multiple of
float32 epsilon times the element's float64 Σ|terms| for a sum) and against the existing tests' figure in their
max-scaled form as a cap; sampled indices and the quantiles exactly. Each test prints the fraction of both it used.
The kernels run through sdreamer.kernels / sdreamer.ops, and through nat.call where only the C ABI admits the arm
(null gradients, accumulate flags, no workspace, a device seed).
"""
import numpy as np
import pytest
import torch

import rowop_models as rm
from oracle import noise as nz

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 12345.0  # fills the bytes a kernel must leave alone


def _d(t):
    return t.to(DEV).contiguous()


def _h(t):
    return t.detach().cpu().numpy()


def _check(fam, got, ref, what):
    print(fam, what, rm.summary(rm.ratios(fam, got, ref)))
    rm.compare(fam, got, ref, f"{fam} {what}")


def test_arm_functions_match_the_library():
    from sdreamer import _native as nat
    for c in rm.RMS_CASES:
        assert rm.rms_bwd_blocks(c.M, c.N) == nat.fns["sd_rmsnorm_bwd_blocks"](c.M, c.N), c.name
    for c in rm.COLSUM_CASES:
        assert rm.colsum_chunks(c.R) == nat.fns["sd_colsum_chunks"](c.R), c.name


# ------------------------------------------------------------------------------------------------ RMSNorm + SiLU
def _block(c, kind, fill=None):
    """the (M, N) tensor `kind` lives in: contiguous, or a column block of a wider SENT-filled buffer"""
    width, col0 = c.blocks()[kind]
    if width == c.N:
        return (torch.full((c.M, c.N), SENT, device=DEV) if fill is None else _d(fill).clone()), None
    buf = torch.full((c.M, width), SENT, device=DEV)
    t = buf[:, col0:col0 + c.N]
    if fill is not None:
        t.copy_(fill)
    return t, buf


def _outside_untouched(c, kind, buf):
    if buf is None:
        return
    width, col0 = c.blocks()[kind]
    keep = torch.ones(width, dtype=torch.bool, device=DEV)
    keep[col0:col0 + c.N] = False
    assert bool((buf[:, keep] == SENT).all()), f"{c.name}: wrote outside the {kind} block"


def run_rms(c, act):
    from sdreamer import kernels as K
    i = rm.rms_inputs(c)
    x, w = _d(i["x"]), _d(i["w"])
    fwd_arm, bwd_arm = c.arms()
    y, ybuf = _block(c, "y")
    assert x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
    assert (y.data_ptr() % 16 == 0) == (c.blocks()["y"][1] % 4 == 0)
    _, rstd = K.rmsnorm_fwd(x, w, act=act, y=y, eps=c.eps)
    _outside_untouched(c, "y", ybuf)
    out = {"y": _h(y), "rstd": _h(rstd)}
    if not c.bwd:
        return out
    dy, dybuf = _block(c, "dy", i["dy"])
    dx, dxbuf = _block(c, "dx", i["dx0"] if c.acc_dx else None)
    dw = None if c.dw is None else _d(i["dw0"]).clone() if c.dw == "acc" else torch.full((c.N,), SENT, device=DEV)
    K.rmsnorm_bwd(x, w, rstd, dy, act=act, dx=dx, dw=dw, accumulate_dx=c.acc_dx, accumulate_dw=c.dw == "acc")
    _outside_untouched(c, "dx", dxbuf)
    _outside_untouched(c, "dy", dybuf)
    out["dx"] = _h(dx)
    if dw is not None:
        out["dw"] = _h(dw)
    return out


@pytest.mark.parametrize("name", [c.name for c in rm.RMS_CASES])
def test_rmsnorm_silu(name):
    c = rm.RMS[name]
    for act in (0, 1):
        _check("rms", run_rms(c, act), rm.reference("rms", c, act), f"{name} act={act} arms={c.arms()}")


# ------------------------------------------------------------------------------------------------ column sums
def run_colsum(c):
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    i = rm.colsum_inputs(c)
    buf = _d(i["buf"])
    before = buf.clone()
    x = buf[:, i["col0"]:i["col0"] + c.N]
    out = _d(i["out0"]).clone() if c.accumulate else torch.full((c.N,), SENT, device=DEV)
    if c.ws:
        K.colsum(x, out, accumulate=c.accumulate)
    else:
        nat.call("sd_colsum", K.p(x), K.p(out), c.R, c.N, x.stride(0), int(c.accumulate), K.stream())
    assert torch.equal(buf, before)
    return {"out": _h(out)}


@pytest.mark.parametrize("name", [c.name for c in rm.COLSUM_CASES])
def test_colsum(name):
    c = rm.COLSUM[name]
    _check("colsum", run_colsum(c), rm.reference("colsum", c), f"{name} arm={c.arm()}")


# ------------------------------------------------------------------------------------------------ teamed heads
def run_sample(c):
    from sdreamer import kernels as K
    i = rm.sample_inputs(c)
    lg = _d(i["logits"])
    idx = torch.full((c.groups,), -1, dtype=torch.int32, device=DEV)
    ent = torch.empty(c.groups, device=DEV)
    args = (c.K, rm.UNIMIX, c.seed, nz.STREAM_IMG, rm.SAMPLE_STEP, rm.SAMPLE_OFFSET)
    st = K.onehot_sample(lg, *args, index=idx, entropy=ent)
    ent_only = K.onehot_entropy(lg, c.K, rm.UNIMIX)  # out = index = 0
    assert torch.equal(ent_only, ent)
    assert torch.equal(st.argmax(-1).int(), idx) and bool((st.sum(-1) - 1).abs().max() < 1e-6)
    dl = K.onehot_sample_bwd(lg, _d(i["dout"]), *args)
    dl_acc = K.onehot_sample_bwd(lg, _d(i["dout"]), *args, dlogits=_d(i["dl0"]).clone(), accumulate=True)
    return {"value": _h(st), "index": _h(idx), "entropy": _h(ent), "dlogits": _h(dl), "dlogits_acc": _h(dl_acc)}


@pytest.mark.parametrize("name", [c.name for c in rm.TEAM_CASES])
def test_onehot_sample(name):
    c = rm.TEAMC[name]
    _check("sample", run_sample(c), rm.reference("sample", c), f"{name} team={rm.team(c.K)}")


def test_onehot_sample_device_seed_bit_equal():
    """the seed split between the host argument and a device seed_ptr (graph replay) equals the host-only seed"""
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    c = rm.TEAMC["K16-g35"]
    i = rm.sample_inputs(c)
    lg, dout = _d(i["logits"]), _d(i["dout"])
    args = (c.K, rm.UNIMIX, c.seed, nz.STREAM_IMG, rm.SAMPLE_STEP, rm.SAMPLE_OFFSET)
    st, dl = K.onehot_sample(lg, *args), K.onehot_sample_bwd(lg, dout, *args)
    part = torch.tensor([1234], dtype=torch.int64, device=DEV)
    st2, dl2 = torch.empty_like(st), torch.empty_like(dl)
    nat.call("sd_onehot_sample_fwd", K.p(lg), K.p(st2), 0, 0, c.groups, c.K, rm.UNIMIX, c.seed - 1234, nz.STREAM_IMG,
             rm.SAMPLE_STEP, rm.SAMPLE_OFFSET, K.p(part), K.stream())
    nat.call("sd_onehot_sample_bwd", K.p(lg), K.p(dout), K.p(dl2), c.groups, c.K, rm.UNIMIX, c.seed - 1234,
             nz.STREAM_IMG, rm.SAMPLE_STEP, rm.SAMPLE_OFFSET, 0, K.p(part), K.stream())
    assert torch.equal(st, st2) and torch.equal(dl, dl2)
    other = K.onehot_sample(lg, c.K, rm.UNIMIX, c.seed - 1234, nz.STREAM_IMG, rm.SAMPLE_STEP, rm.SAMPLE_OFFSET)
    assert not torch.equal(other, st)  # the device part does enter


def run_logp(c):
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    from sdreamer import ops
    i = rm.sample_inputs(c)
    lg, act = _d(i["logits"]).requires_grad_(), _d(i["action"])
    g1, g2 = _d(i["glogp"]), _d(i["gent"])
    lp, ent = ops.OneHotLogProbEntFn.apply(lg, act, rm.UNIMIX)
    (lp * g1 + ent * g2).sum().backward()
    out = {"logp": _h(lp), "ent": _h(ent), "dl_both": _h(lg.grad)}
    for key, a, b in (("dl_lp", g1, None), ("dl_ent", None, g2)):
        dl = torch.full_like(lg, SENT)
        nat.call("sd_onehot_logp_ent_bwd", K.p(lg), K.p(act), K.p(a), K.p(b), K.p(dl), c.groups, c.K, rm.UNIMIX,
                 K.stream())
        out[key] = _h(dl)
    return out


@pytest.mark.parametrize("name", [c.name for c in rm.TEAM_CASES])
def test_onehot_logp_ent(name):
    c = rm.TEAMC[name]
    _check("logp", run_logp(c), rm.reference("logp", c), f"{name} team={rm.team(c.K)}")


def _kl_bwd(c, i, kl, g_rep, g_dyn, d_post, d_prior, acc_post=0, acc_prior=0):
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    post, prior = _d(i["post"]), _d(i["prior"])  # named: both alive until the launch is queued
    nat.call("sd_kl_bwd", K.p(post), K.p(prior), K.p(kl), K.p(g_rep), K.p(g_dyn), i["free"], K.p(d_post), K.p(d_prior),
             c.rows, c.S, c.K, acc_post, acc_prior, K.stream())


def run_kl(c):
    from sdreamer import kernels as K
    from sdreamer import ops
    i = rm.kl_inputs(c)
    p, q = _d(i["post"]).requires_grad_(), _d(i["prior"]).requires_grad_()
    g_rep, g_dyn = _d(i["g_rep"]), _d(i["g_dyn"])
    dyn, rep = ops.KLFn.apply(p, q, i["free"], c.S, c.K)
    (g_rep * rep + g_dyn * dyn).sum().backward()
    kl = K.kl_rows(p.detach(), q.detach(), c.S, c.K)
    out = {"kl": _h(kl), "dyn": _h(dyn), "rep": _h(rep), "d_post": _h(p.grad), "d_prior": _h(q.grad)}
    dpa, dqa = _d(i["dpost0"]).clone(), _d(i["dprior0"]).clone()
    _kl_bwd(c, i, kl, g_rep, g_dyn, dpa, dqa, 1, 1)
    out.update(d_post_acc=_h(dpa), d_prior_acc=_h(dqa))
    return out, kl


@pytest.mark.parametrize("name", [c.name for c in rm.KL_CASES])
def test_kl(name):
    c = rm.KL[name]
    got, kl = run_kl(c)
    ref = rm.reference("kl", c)
    _check("kl", got, ref, f"{name} team={rm.team(c.K)}")
    below = ref["kl"] < rm.kl_inputs(c)["free"]
    assert (got["d_post"][below] == 0).all() and (got["d_prior"][below] == 0).all()  # exactly zero below free
    if c.rows > 5:
        return
    # each of g_rep, g_dyn, d_post, d_prior null in turn: a null upstream gradient writes zeros, a null output is not
    # written and the other is unchanged
    i = rm.kl_inputs(c)
    g_rep, g_dyn = _d(i["g_rep"]), _d(i["g_dyn"])
    new = lambda: torch.full((c.rows, c.S * c.K), SENT, device=DEV)  # noqa: E731
    for null in ("g_rep", "g_dyn", "d_post", "d_prior"):
        dp, dq = (None if null == "d_post" else new()), (None if null == "d_prior" else new())
        _kl_bwd(c, i, kl, None if null == "g_rep" else g_rep, None if null == "g_dyn" else g_dyn, dp, dq)
        if dp is not None:
            assert np.array_equal(_h(dp), np.zeros_like(got["d_post"]) if null == "g_rep" else got["d_post"]), null
        if dq is not None:
            assert np.array_equal(_h(dq), np.zeros_like(got["d_prior"]) if null == "g_dyn" else got["d_prior"]), null


# ------------------------------------------------------------------------------------------------ two-hot family
def run_twohot(c):
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    from sdreamer import ops
    i = rm.twohot_inputs(c)
    bins, t, g = _d(i["bins"]), _d(i["target"]), _d(i["g"])
    lg = _d(i["logits"]).requires_grad_()
    lp = ops.TwoHotLogProbFn.apply(lg, bins, t)
    lp.backward(g)
    dl_acc = _d(i["dl0"]).clone()
    nat.call("sd_twohot_logp_bwd", K.p(lg), K.p(bins), K.p(t), K.p(g), K.p(dl_acc), c.rows, c.NB, 1, K.stream())
    out = {"logp": _h(lp), "dlogits": _h(lg.grad), "dlogits_acc": _h(dl_acc)}
    if c.NB % 2 == 1:
        out["mode"] = _h(K.twohot_mode(lg.detach(), bins)).reshape(-1)
        out["dmode"] = _h(K.twohot_mode_bwd(lg.detach(), bins, g))
    return out


@pytest.mark.parametrize("name", [c.name for c in rm.TWOHOT_CASES])
def test_twohot(name):
    c = rm.TWOHOT[name]
    _check("twohot", run_twohot(c), rm.reference("twohot", c), name)


def run_repval(c):
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    from sdreamer import ops
    i = rm.repval_inputs(c)
    bins, ret, slow, last = (_d(i[k]) for k in ("bins", "ret", "slow", "last"))
    lg = _d(i["logits"]).requires_grad_()
    loss = ops.RepvalLossFn.apply(lg, bins, ret, slow, last)
    torch.autograd.backward(loss, torch.full((), rm.REPVAL_GSCALE, device=DEV))
    rows = torch.empty(c.B * c.Tr, device=DEV)
    nat.call("sd_repval_loss_fwd", K.p(lg), K.p(bins), K.p(ret), K.p(slow), K.p(last), K.p(rows), c.B, c.Tl, c.Tr,
             c.NB, K.stream())
    assert bool((lg.grad[:, c.Tr:] == 0).all())  # the steps without a return
    return {"rows": _h(rows), "loss": _h(loss.reshape(1)), "dlogits": _h(lg.grad.reshape(-1, c.NB))}


@pytest.mark.parametrize("name", [c.name for c in rm.REPVAL_CASES])
def test_repval_loss(name):
    c = rm.REPVAL[name]
    _check("repval", run_repval(c), rm.reference("repval", c), name)


def run_imag_ac(c):
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    i = rm.imag_ac_inputs(c)
    t = {k: _d(v) for k, v in i.items()}
    HN = c.H * c.N
    rows_v, rows_p, adv = torch.empty(HN, device=DEV), torch.empty(HN, device=DEV), torch.empty(c.N, c.H, device=DEV)
    nat.call("sd_imag_ac_loss_fwd", K.p(t["vl"]), K.p(t["bins"]), K.p(t["ret"]), K.p(t["slow"]), K.p(t["weight"]),
             K.p(t["val"]), K.p(t["scale"].reshape(1)), K.p(t["logpi"]), K.p(t["ent"]), rm.AC_COEF, c.N, c.H, c.H1,
             c.NB, K.p(rows_v), K.p(rows_p), K.p(adv), K.stream())
    out = {"rows_v": _h(rows_v), "rows_p": _h(rows_p), "adv": _h(adv), "policy": _h(K.device_mean(rows_p).reshape(1)),
           "value": _h(K.device_mean(rows_v).reshape(1))}
    gp, gv = torch.tensor([rm.AC_GP], device=DEV), torch.tensor([rm.AC_GV], device=DEV)
    res = {}
    for key, a, b in (("both", gp, gv), ("gp_null", None, gv), ("gv_null", gp, None)):
        dvl = torch.full((HN, c.NB), SENT, device=DEV)
        dlp, den = torch.full((HN,), SENT, device=DEV), torch.full((HN,), SENT, device=DEV)
        nat.call("sd_imag_ac_loss_bwd", K.p(t["vl"]), K.p(t["bins"]), K.p(t["ret"]), K.p(t["slow"]), K.p(t["weight"]),
                 K.p(adv), K.p(a), K.p(b), rm.AC_SP, rm.AC_SV, rm.AC_COEF, c.N, c.H, c.H1, c.NB, K.p(dvl), K.p(dlp),
                 K.p(den), K.stream())
        res[key] = (_h(dvl), _h(dlp), _h(den))
    out.update(dvl=res["both"][0], dlogpi=res["both"][1], dent=res["both"][2])
    # a null upstream gradient zeroes its side and leaves the other side's bits
    assert not res["gp_null"][1].any() and not res["gp_null"][2].any() and np.array_equal(res["gp_null"][0], out["dvl"])
    assert not res["gv_null"][0].any() and np.array_equal(res["gv_null"][1], out["dlogpi"])
    assert np.array_equal(res["gv_null"][2], out["dent"])
    return out


@pytest.mark.parametrize("name", [c.name for c in rm.IMAG_AC_CASES])
def test_imag_ac_loss(name):
    c = rm.IMAG_AC[name]
    _check("imag_ac", run_imag_ac(c), rm.reference("imag_ac", c), name)


# ------------------------------------------------------------------------------------------------ pointwise heads
def run_bnormal(c):
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    from sdreamer import ops
    i = rm.bn_inputs(c)
    x, a, g1, g2 = _d(i["x"]).requires_grad_(), _d(i["action"]), _d(i["glogp"]), _d(i["gent"])
    lp, ent = ops.BNormalLogProbEntFn.apply(x, a, rm.BN_MIN_STD, rm.BN_MAX_STD)
    (lp * g1 + ent * g2).sum().backward()
    out = {"logp": _h(lp), "ent": _h(ent), "dx_both": _h(x.grad)}
    for key, u, v in (("dx_lp", g1, None), ("dx_ent", None, g2)):
        dx = torch.full_like(x, SENT)
        nat.call("sd_bnormal_logp_ent_bwd", K.p(x), K.p(a), K.p(u), K.p(v), K.p(dx), c.rows, c.A, rm.BN_MIN_STD,
                 rm.BN_MAX_STD, K.stream())
        out[key] = _h(dx)
    return out


@pytest.mark.parametrize("name", [c.name for c in rm.BN_CASES])
def test_bnormal_logp_ent(name):
    c = rm.BN[name]
    _check("bnormal", run_bnormal(c), rm.reference("bnormal", c), name)


def run_bernoulli(rows):
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    from sdreamer import ops
    i = rm.bern_inputs(rows)
    lg, v, g = _d(i["logit"]).requires_grad_(), _d(i["value"]), _d(i["g"])
    lp = ops.BernoulliLogProbFn.apply(lg.unsqueeze(-1), v.unsqueeze(-1))
    lp.backward(g)
    mean, mean_only = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    lp2 = torch.empty(rows, device=DEV)
    nat.call("sd_bernoulli_fwd", K.p(lg), K.p(v), K.p(lp2), K.p(mean), rows, K.stream())
    nat.call("sd_bernoulli_fwd", K.p(lg), 0, 0, K.p(mean_only), rows, K.stream())  # logp null: the mean alone
    assert torch.equal(lp2, lp.detach()) and torch.equal(mean, mean_only)
    return {"logp": _h(lp), "mean": _h(mean), "dlogit": _h(lg.grad)}


@pytest.mark.parametrize("rows", rm.BERN_ROWS)
def test_bernoulli(rows):
    _check("bernoulli", run_bernoulli(rows), rm.reference("bernoulli", rows), str(rows))


def run_gru(c):
    from sdreamer import kernels as K
    i = rm.gru_inputs(c)
    gates, h, dout = _d(i["gates"]), _d(i["h"]), _d(i["dout"])
    out = K.gru_fwd(gates, h, c.G)
    dg, dh = K.gru_bwd(gates, h, dout, c.G)
    dg2, dh_acc = K.gru_bwd(gates, h, dout, c.G, dh=_d(i["dh0"]).clone(), accumulate_dh=True)
    assert torch.equal(dg, dg2)
    return {"out": _h(out), "dgates": _h(dg), "dh": _h(dh), "dh_acc": _h(dh_acc)}


@pytest.mark.parametrize("name", [c.name for c in rm.GRU_CASES])
def test_gru_gates(name):
    c = rm.GRU[name]
    _check("gru", run_gru(c), rm.reference("gru", c), name)


# ------------------------------------------------------------------------------------------------ λ-return
def run_lret(c, strided):
    """row-major, or every strided read: time-major reward / boot, the continue logit a column of a wider matrix"""
    from sdreamer import kernels as K
    i = rm.lret_inputs(c)
    N, T = c.N, c.T
    boot = i["boot"] if c.form != "imag" else i["value"]
    kw = {}
    if c.form != "imag":
        kw.update(term=_d(i["term"]), last=_d(i["last"]))
    if c.form != "replay":
        kw.update(cont_out=torch.full((N, T), SENT, device=DEV), weight_out=torch.full((N, T), SENT, device=DEV))
    if not strided:
        rew, bt = _d(i["reward"]), _d(boot)
        if c.form != "replay":
            kw["cont_logit"] = _d(i["cont_logit"])
    else:
        rew, bt = _d(i["reward"].t()).t(), _d(boot.t())
        kw.update(boot_row_stride=1, boot_t_stride=N)
        if c.form != "replay":
            wide = torch.full((T * N, 3), SENT, device=DEV)
            wide[:, 1] = _d(i["cont_logit"].t()).reshape(-1)
            kw["cont_logit"] = wide[:, 1].view(T, N).t()
    ret = K.lambda_return(rew, bt, rm.DISC, c.lamb, **kw)
    out = {"ret": _h(ret)}
    if c.form != "replay":
        out.update(cont=_h(kw["cont_out"]), weight=_h(kw["weight_out"]))
    return out


@pytest.mark.parametrize("name", [c.name for c in rm.LRET_CASES])
def test_lambda_return(name):
    c = rm.LRET[name]
    got = run_lret(c, False)
    assert got["ret"].shape == (c.N, c.T - 1)
    _check("lret", got, rm.reference("lret", c), f"{name} arm={c.arm()}")
    tm = run_lret(c, True)
    assert rm.same_bits(got, tm), "the strided, time-major reads differ from the row-major ones"


# ------------------------------------------------------------------------------------------------ ReturnEMA
def run_ema(c):
    from sdreamer import kernels as K
    i = rm.ema_inputs(c)
    ema = torch.tensor(rm.EMA0, device=DEV)
    out = {}
    for k in ("1", "2"):  # the second call continues from the in-place EMA
        os_, q = torch.full((2,), SENT, device=DEV), torch.full((2,), SENT, device=DEV)
        K.return_ema(_d(i["x" + k]), ema, os_, quantiles=q, alpha=rm.EMA_ALPHA)
        out["q" + k], out["ema" + k], out["os" + k] = _h(q), _h(ema), _h(os_)
    return out


@pytest.mark.parametrize("name", [c.name for c in rm.EMA_CASES])
def test_return_ema(name):
    c = rm.EMA[name]
    _check("ema", run_ema(c), rm.reference("ema", c), f"{name} arm={rm.ema_arm(c.n)}")


# ------------------------------------------------------------------------------------------------ refusals
def test_entry_points_refuse_what_they_cannot_run():
    """Every call below returns before any launch (SD_ESHAPE / SD_EARG -> NativeError), so none reaches the device;
    the buffers are real and large enough for the nearest admitted shape all the same."""
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    z = torch.zeros(4096, device=DEV)
    zi = torch.zeros(64, dtype=torch.int32, device=DEV)
    P, s = K.p(z), K.stream()

    def refused(name, *args):
        with pytest.raises(nat.NativeError):
            nat.call(name, *args)

    for k in (0, 65):
        refused("sd_onehot_sample_fwd", P, P, K.p(zi), P, 2, k, 0.01, 0, 0, 0, 0, 0, s)
        refused("sd_onehot_sample_bwd", P, P, P, 2, k, 0.01, 0, 0, 0, 0, 0, 0, s)
        refused("sd_onehot_logp_ent_fwd", P, P, P, P, 2, k, 0.01, s)
        refused("sd_onehot_logp_ent_bwd", P, P, P, P, P, 2, k, 0.01, s)
        refused("sd_kl_fwd", P, P, P, P, P, 1.0, 2, 2, k, s)
        refused("sd_kl_bwd", P, P, P, P, P, 1.0, P, P, 2, 2, k, 0, 0, s)
    for nb in (0, 257):
        refused("sd_twohot_mode", P, P, P, 2, nb, s)
        refused("sd_twohot_mode_bwd", P, P, P, P, 2, nb, s)
        refused("sd_twohot_logp_fwd", P, P, P, P, 2, nb, s)
        refused("sd_twohot_logp_bwd", P, P, P, P, P, 2, nb, 0, s)
        refused("sd_repval_loss_fwd", P, P, P, P, P, P, 2, 3, 2, nb, s)
        refused("sd_repval_loss_bwd", P, P, P, P, P, P, 0.25, P, 2, 3, 2, nb, s)
        refused("sd_imag_ac_loss_fwd", P, P, P, P, P, P, P, P, P, 0.0, 2, 2, 3, nb, P, P, P, s)
        refused("sd_imag_ac_loss_bwd", P, P, P, P, P, P, P, P, 1.0, 1.0, 0.0, 2, 2, 3, nb, P, P, P, s)
    refused("sd_twohot_mode", P, P, P, 2, 254, s)
    refused("sd_twohot_mode_bwd", P, P, P, P, 2, 254, s)
    for n in (0, 4097):
        refused("sd_rmsnorm_fwd", P, P, P, P, 1, n, 1e-4, 1, s)
        refused("sd_rmsnorm_bwd", P, P, P, P, P, P, P, 1, n, 1, 0, 1, s)
    refused("sd_rmsnorm_fwd_ld", P, P, P, 15, P, 2, 16, 1e-4, 1, s)  # ldy < N
    refused("sd_rmsnorm_bwd_ldx", P, P, P, P, 16, P, 15, P, P, 2, 16, 1, 0, 1, s)  # ldx < N
    refused("sd_rmsnorm_bwd_ldx", P, P, P, P, 15, P, 16, P, P, 2, 16, 1, 0, 1, s)  # ldy < N
    refused("sd_repval_loss_fwd", P, P, P, P, P, P, 2, 2, 3, 255, s)  # Tr > Tl
    refused("sd_repval_loss_bwd", P, P, P, P, P, P, 0.25, P, 2, 2, 3, 255, s)
    for h1 in (1, 2):  # H1 <= H
        refused("sd_imag_ac_loss_fwd", P, P, P, P, P, P, P, P, P, 0.0, 2, 2, h1, 255, P, P, P, s)
        refused("sd_imag_ac_loss_bwd", P, P, P, P, P, P, P, P, 1.0, 1.0, 0.0, 2, 2, h1, 255, P, P, P, s)
    refused("sd_lambda_return", P, 0, 0, 0, P, 4, 1, P, 0, 0, 2, 4, 0.99, 0.95, s)  # neither term nor cont_logit
    refused("sd_return_ema", P, 0, P, P, P, 0.01, 0.05, 0.95, s)
    # empty work is no error: A = 0 (the bounded normal family), as its siblings answer rows = 0
    for name, args in (("sd_bnormal_sample", (P, P, 2, 0, 0.1, 1.0, 0, 0, 0, 0, 0, s)),
                       ("sd_bnormal_sample_bwd", (P, P, P, P, 2, 0, 0.1, 1.0, 0, 0, 0, 0, 0, s)),
                       ("sd_bnormal_logp_ent_fwd", (P, P, P, P, 2, 0, 0.1, 1.0, s)),
                       ("sd_bnormal_logp_ent_bwd", (P, P, P, P, P, 2, 0, 0.1, 1.0, s))):
        nat.call(name, *args)
    torch.cuda.synchronize()
    assert not z.any() and not zi.any()
