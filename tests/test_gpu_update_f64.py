"""The tail of the update — csrc/misc.hip (Barlow single-GPU and data-parallel, InfoNCE, the metric vector, the weighted
loss total, input preparation, replay slices) and csrc/optim.hip (AGC + LaProp, Polyak) — against float64 at the
smallest shapes that reach every arm of their dispatch (tests/update_models.py holds the tables, inputs, references
and comparison; tests/test_update_parity_cpu.py checks on the CPU that the tables reach the arms, that the float32
restatement passes with room and that planted faults fail; DESIGN.md § 2.4 lists the cases with the arm each reaches
and the measured figures).

Every output is compared elementwise (parity.assert_close: atol = tol * max(|ref_i|, 1), or a stated multiple of
float32 epsilon times the element's float64 Σ|terms| for a sum) and against the existing tests' figure in its own form
as a cap; copies, selections, indices, min and max exactly. Each test prints the fraction of both it used. The kernels
run through sdreamer.ops / kernels / parallel / optim, and through nat.call where only the C ABI admits the arm
(ld > ncol, null pointers, null grad_norms, img = NULL).
"""
import ctypes

import numpy as np
import pytest
import torch

import parity
import update_models as um

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 12345.0  # fills the bytes a kernel must leave alone


def _d(t):
    return torch.as_tensor(t).to(DEV).contiguous()


def _h(t):
    return t.detach().cpu().numpy()


def _check(fam, got, ref, what):
    assert set(got) == set(um.outputs(ref)), (what, set(got) ^ set(um.outputs(ref)))  # no output left out
    print(fam, what, um.summary(um.ratios(fam, got, ref)))
    um.compare(fam, got, ref, f"{fam} {what}")


# ------------------------------------------------------------------------------------------------ Barlow
def _barlow_fn(c, i):
    from sdreamer import kernels as K
    from sdreamer import ops
    nat, p, s = K.nat, K.p, K.stream()
    N, E, lam = c.Nr, c.E, um.BARLOW_LAMBD
    x1, x2 = _d(i["x1"]), _d(i["x2"])
    g = torch.full((1,), um.BARLOW_G, device=DEV)
    # ops.BarlowFn's launches one by one (its intermediates are not returned), then the function itself: the same bits
    m, sd, n = torch.empty(2, E, device=DEV), torch.empty(2, E, device=DEV), []
    for k, x in enumerate((x1, x2)):
        nat.call("sd_colstats", p(x), N, E, p(m[k]), p(sd[k]), s)
        n.append(torch.empty_like(x))
        nat.call("sd_standardize", p(x), p(m[k]), p(sd[k]), p(n[k]), N, E, um.BARLOW_EPS, s)
    cc = K.mm(n[0].t(), n[1], alpha=1.0 / N)
    part, loss = torch.empty(2 * um.BARLOW_PARTIAL_BLOCKS, device=DEV), torch.empty(1, device=DEV)
    nat.call("sd_barlow_loss", p(cc), E, lam, p(part), um.BARLOW_PARTIAL_BLOCKS, p(loss), s)
    dc = torch.empty_like(cc)
    nat.call("sd_barlow_dc", p(cc), p(g), p(dc), E, lam, s)
    dn1 = K.mm(n[1], dc.t(), alpha=1.0 / N)
    dx1, sbwd = torch.empty_like(x1), torch.full_like(x1, SENT)
    nat.call("sd_standardize_bwd", p(x1), p(m[0]), p(sd[0]), p(dn1), p(dx1), N, E, um.BARLOW_EPS, s)
    nat.call("sd_standardize_bwd", p(x1), p(m[0]), p(sd[0]), p(_d(i["dnr"])), p(sbwd), N, E, um.BARLOW_EPS, s)
    xg = x1.clone().requires_grad_()
    lf = ops.BarlowFn.apply(xg, x2, lam)
    lf.backward(g[0])
    assert torch.equal(lf.reshape(1), loss) and torch.equal(xg.grad, dx1)
    return {"mean": m, "std": sd, "n1": n[0], "n2": n[1], "c": cc, "loss": loss, "dc": dc, "dx1": dx1, "sbwd": sbwd}


def _barlow_steps(c, i):
    from sdreamer import kernels as K
    from sdreamer import parallel
    BS, nat, p, s = parallel.BarlowSteps, K.nat, K.p, K.stream()
    N, E, lam, world = c.Nr, c.E, um.BARLOW_LAMBD, c.world
    Nt = float(N)
    rows, lo = [], 0
    for r in c.shards():
        rows.append(slice(lo, lo + r))
        lo += r
    shards = [(_d(i["x1"][r]), _d(i["x2"][r])) for r in rows]
    sums = sum(BS.colsums(a, b) for a, b in shards)  # all-reduce 1
    cen = [BS.center(a, b, sums, Nt) for a, b in shards]
    stats = sum(st for _, _, st in cen)  # all-reduce 2
    g = torch.full((), um.BARLOW_G, device=DEV)
    dcr, cr, z2r, s1r, s0r, Ar, sums_in = (_d(i[k]) for k in ("dcr", "cr", "z2r", "s1r", "s0r", "Ar", "sums_in"))
    per = []
    for (a, _), (_, d2, _), r in zip(shards, cen, rows):
        cc, st, n2, z2 = BS.finish(stats, sums, Nt, d2)
        xg = a.clone().requires_grad_()
        ld = parallel._DistBarlowLoss.apply(xg, cc, sums, st, n2, z2, lam, Nt, world)
        ld.backward(g)
        dc = torch.empty_like(cc)
        nat.call("sd_barlow_dc", p(cc), p(g.reshape(1)), p(dc), E, lam, s)
        s0, A = torch.full((E,), SENT, device=DEV), torch.full((E,), SENT, device=DEV)
        nat.call("sd_barlow_rowstats", p(dc), p(cc), p(z2), p(st[0]), Nt, E, p(s0), p(A), s)
        dxd = torch.full_like(a, SENT)
        nat.call("sd_barlow_dist_dx", p(a), p(_d(i["dnr"][r])), p(sums_in), p(s1r), p(s0r), p(Ar), Nt, float(world),
                 a.shape[0], E, p(dxd), s)
        per.append(dict(c=cc, std=st, n2=n2, z2=z2, loss=ld.detach().reshape(1), dc=dc, s0=s0, A=A,
                        dx1=xg.grad / world, dxd=dxd))
    for q in per[1:]:  # every rank holds the same global quantities
        assert all(torch.equal(q[k], per[0][k]) for k in ("c", "std", "z2", "loss", "dc", "s0", "A"))
    s0d, Ad = torch.full((E,), SENT, device=DEV), torch.full((E,), SENT, device=DEV)
    nat.call("sd_barlow_rowstats", p(dcr), p(cr), p(z2r), p(s1r), Nt, E, p(s0d), p(Ad), s)
    out = {k: per[0][k] for k in ("c", "std", "z2", "loss", "dc", "s0", "A")}
    out.update({k: torch.cat([q[k] for q in per]) for k in ("n2", "dx1", "dxd")})
    out.update(sums=sums, d1=torch.cat([d for d, _, _ in cen]), d2=torch.cat([d for _, d, _ in cen]),
               q=stats[:2 * E].view(2, E), craw=stats[2 * E:].view(E, E), s0d=s0d, Ad=Ad)
    return out


def run_barlow(c):
    i = um.barlow_inputs(c)
    out = _barlow_fn(c, i) if c.mode == "fn" else _barlow_steps(c, i)
    return {k: _h(v) for k, v in out.items()}


@pytest.mark.parametrize("name", [c.name for c in um.BARLOW_CASES])
def test_barlow(name):
    c = um.BARLOW[name]
    _check("barlow", run_barlow(c), um.reference("barlow", c),
           f"{name} blocks={um.col_blocks(c.E)} partials={um.row_partials(c.shards()[0])}")


# ------------------------------------------------------------------------------------------------ InfoNCE
def run_infonce(c):
    from sdreamer import kernels as K
    from sdreamer import ops
    nat, p, s = K.nat, K.p, K.stream()
    i = um.nce_inputs(c)
    n, ncol, ld = c.n, c.ncol, c.ncol + c.ld_extra
    buf = torch.full((n, ld), SENT, device=DEV)
    buf[:, :ncol] = _d(i["logits"])
    row, lse, loss = (torch.full((k,), SENT, device=DEV) for k in (n, n, 1))
    nat.call("sd_infonce_fwd", p(buf), ld, n, ncol, c.off, p(row), p(lse), p(loss), s)
    g = torch.full((1,), um.NCE_G, device=DEV)
    dl = torch.full((n, ncol), SENT, device=DEV)
    nat.call("sd_infonce_bwd", p(buf), ld, n, ncol, c.off, p(lse), p(g), 1.0 / n, p(dl), s)
    assert bool((buf[:, ncol:] == SENT).all())
    x1 = _d(i["x1"]).requires_grad_()
    lf = ops.InfoNCEFn.apply(x1, _d(i["x2g"]), c.off)
    lf.backward(g[0])
    return {"lse": _h(lse), "row_loss": _h(row), "loss": _h(loss), "dlogits": _h(dl), "fn_loss": _h(lf.reshape(1)),
            "dx1": _h(x1.grad)}


@pytest.mark.parametrize("name", [c.name for c in um.NCE_CASES])
def test_infonce(name):
    c = um.NCE[name]
    _check("infonce", run_infonce(c), um.reference("infonce", c), name)


# ------------------------------------------------------------------------------------------------ metric vector
def run_stats(c):
    from sdreamer import kernels as K
    i = um.stat_inputs(c)
    A, D, C = _d(i["a"]), _d(i["d"]), torch.tensor(um.STAT_C, device=DEV)
    sub, div = torch.tensor([um.STAT_SUB], device=DEV), torch.tensor([um.STAT_DIV], device=DEV)
    vals = list(K.tensorstats(A, "a").values()) + [
        K.Stat(A, sub=sub, div=div), K.Stat(A, K.STAT_STD, sub=sub, div=div),
        K.Stat(C) + K.Stat(A, scale=0.5) + K.Stat(D, K.STAT_MAX, scale=-2.0)]  # three requests into one slot
    v = _h(K.metric_vector(vals))
    out = {"mean": v[0:1], "min": v[2:3], "max": v[3:4], "affine": v[4:5], "combo": v[6:7]}
    if c.n > 1:
        out.update(std=v[1:2], affine_std=v[5:6])
    else:
        assert np.isnan(v[5])
        out["nan"] = v[1:2]
    return out


@pytest.mark.parametrize("name", [c.name for c in um.STAT_CASES])
def test_metric_vector(name):
    c = um.STAT[name]
    _check("stats", run_stats(c), um.reference("stats", c), f"{name} chunks={um.stat_chunks(c.n)}")


# ------------------------------------------------------------------------------------------------ loss terms
def run_loss_terms(c):
    from sdreamer import kernels as K
    i = um.lt_inputs(c)
    k = len(c.ns)
    xs = [_d(x) for x in i["xs"]]
    coefs, scales = um.LT_COEFS[:k], um.LT_SCALES[:k]
    means, total = torch.full((k,), SENT, device=DEV), torch.full((1,), SENT, device=DEV)
    K.loss_terms(xs, coefs, scales, means, total)
    total2 = torch.full((1,), SENT, device=DEV)
    K.loss_terms(xs, coefs, scales, None, total2)  # means null
    assert torch.equal(total, total2)
    out = {"means": _h(means), "total": _h(total)}
    # the total is the ordered float32 sum of the scaled means, bit for bit
    assert out["total"][0] == um.ordered_total_f32(out["means"], scales), (out["total"], out["means"])
    gt, gm = torch.full((1,), um.LT_GT, device=DEV), _d(i["gm"])
    for var, (a, b) in {"all": (gt, gm), "nogt": (None, gm), "nogm": (gt, None)}.items():
        grads = [torch.full((n,), SENT, device=DEV) for n in c.ns]
        K.loss_terms_bwd(c.ns, coefs, scales, grads, a, b)
        out["grads_" + var] = np.concatenate([_h(g) for g in grads])
        if var == "all":  # one t.g null: that term is skipped, the others are the same bits
            for skip in {0, k - 1}:
                again = [None if j == skip else torch.full((n,), SENT, device=DEV) for j, n in enumerate(c.ns)]
                K.loss_terms_bwd(c.ns, coefs, scales, again, a, b)
                assert all(torch.equal(x, y) for j, (x, y) in enumerate(zip(again, grads)) if j != skip)
    return out


@pytest.mark.parametrize("name", [c.name for c in um.LT_CASES])
def test_loss_terms(name):
    c = um.LT[name]
    _check("loss_terms", run_loss_terms(c), um.reference("loss_terms", c), f"{name} gx={um.loss_terms_gx(max(c.ns))}")


# ------------------------------------------------------------------------------------------------ input preparation
def run_prep(n):
    from sdreamer import kernels as K
    i = um.prep_inputs(n)
    out = {"symlog": _h(K.symlog(_d(i["symlog"]))), "action_norm": _h(K.action_norm(_d(i["action"])))}
    for w in (1, 7):
        for st in (1, 3):
            out[f"mask_rows_w{w}s{st}"] = _h(K.mask_rows(_d(i[f"mx{w}"]), _d(i[f"mask{w}s{st}"]), st))
    la, te, co = K.episode_flags(_d(i["last"]).view(1, n), _d(i["termb"]).view(1, n))
    out.update(last=_h(la).reshape(n), term=_h(te).reshape(n), cont=_h(co).reshape(n))
    for sh in um.U8_SHIFTS:
        tag = f"s{sh:g}"
        out[f"u8_{tag}"] = _h(K.u8_to_f32(_d(i["bytes"]), sh))
        for C, Cp in um.U8_CP:
            key = f"c{C}p{Cp}{tag}"
            img, enc = K.u8_image_inputs(_d(i[f"img{C}"]), Cp, sh, need_f32=sh == 0.0)  # shift 0.5: img = NULL
            out[f"enc_{key}"] = _h(enc)
            if sh == 0.0:
                out[f"img_{key}"] = _h(img)
            q32 = (i[f"img{C}"].float() / 255.0)
            out[f"pad_{key}"] = _h(K.pad_channels(_d(q32), Cp, sh))
    for k in [k for k in out if k.split("_")[0] in ("u8", "img", "enc", "pad")]:  # bit for bit with float32 torch
        head, rest = k.split("_", 1)
        out[f"{head}_f32_{rest}"] = out[k]
    return out


@pytest.mark.parametrize("n", um.PREP_NS)
def test_input_preparation(n):
    got = run_prep(n)
    a, ref = got["action_norm"], um.reference("prep", n)
    x = um.prep_inputs(n)["action"].numpy()
    assert np.array_equal(a[np.abs(x) <= 1], x[np.abs(x) <= 1])  # a / 1 is a
    _check("prep", got, ref, f"n={n}")


# ------------------------------------------------------------------------------------------------ optimiser
def _tensor_index():
    offs, total, *_ = um.arena_layout(um.OPT_SIZES)
    idx = torch.cat([torch.arange(o, o + n) for o, n in zip(offs, um.OPT_SIZES)]).to(DEV)
    pad = torch.ones(total, dtype=torch.bool, device=DEV)
    pad[idx] = False
    return idx, pad


def _new_opt(c):
    from sdreamer.optim import LaProp
    i = um.opt_inputs()
    params = [torch.nn.Parameter(p.clone().to(DEV)) for p in i["p"]]
    opt = LaProp(params, warmup=c.warmup, **um.OPT_HP)
    opt.grad_scale = c.grad_scale
    if c.gate is not None:
        opt.gate = (um.OPT_GATED, torch.full((1,), c.gate, device=DEV))
    opt.zero_grads_after = c.variant == "zg"
    return params, opt


def run_optim(c):
    i = um.opt_inputs()
    params, opt = _new_opt(c)
    a = opt.arena
    assert um.arena_layout(um.OPT_SIZES)[:2] == (a.offsets, a.total)
    idx, pad = _tensor_index()
    out = {}
    for it in range(um.OPT_STEPS):
        for j, g in enumerate(i["g"][it]):
            if c.variant == "zg":
                params[j].grad.add_(g.to(DEV))  # onto the zeros the previous step left
            else:
                params[j].grad.copy_(g.to(DEV))
        prev = a.data.double()
        opt.step()
        k = str(it)
        out["dp" + k] = _h((a.data.double() - prev)[idx])
        out["m" + k], out["v" + k] = _h(opt.exp_avg[idx]), _h(opt.exp_avg_sq[idx])
        out["gn" + k] = _h(opt.grad_norms)
        out["scalars" + k] = _h(opt.scalars[:4])
        for nm, t in (("params", a.data), ("exp_avg", opt.exp_avg), ("exp_avg_sq", opt.exp_avg_sq), ("grads", a.grad)):
            assert not bool(t[pad].any()), f"{c.name} step {it}: the {nm} arena's padding is no longer zero"
        if c.variant == "zg":
            assert not bool(a.grad.any())
    return out


@pytest.mark.parametrize("name", [c.name for c in um.OPT_CASES])
def test_agc_laprop(name):
    c = um.OPT[name]
    ref = um.reference("optim", c)
    got = run_optim(c)
    for it in range(um.OPT_STEPS):  # the scalar state against the oracle's Python floats
        a, b = got[f"scalars{it}"], ref[f"scalars{it}"]
        assert (np.abs(a - b) <= 1e-12 * np.abs(b)).all(), (it, a, b)
    _check("optim", got, ref, name)


def test_agc_laprop_without_grad_norms():
    """grad_norms = NULL runs, and the step is the same bits"""
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    c = um.OPT["w1000-plain"]
    i = um.opt_inputs()
    res = []
    for null in (False, True):
        params, opt = _new_opt(c)
        a = opt.arena
        for j, g in enumerate(i["g"][1]):
            params[j].grad.copy_(g.to(DEV))
        opt.grad_norms.fill_(SENT)
        nat.call("sd_agc_laprop_step", K.p(a.data), K.p(a.grad), K.p(opt.exp_avg), K.p(opt.exp_avg_sq),
                 K.p(a.chunk_beg), K.p(a.chunk_end), K.p(a.chunk_tensor), K.p(a.tensor_chunk0), a.nchunks, a.ntensors,
                 K.p(opt.workspace), K.p(opt.scalars), 0 if null else K.p(opt.grad_norms), opt.agc, opt.pmin,
                 opt.base_lr, opt.warmup, opt.betas[0], opt.betas[1], opt.eps, 1.0, -1, 0, 0, K.stream())
        res.append((a.data.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.grad_norms.clone()))
    assert all(torch.equal(x, y) for x, y in zip(res[0][:3], res[1][:3]))
    assert bool((res[1][3] == SENT).all()) and not bool((res[0][3] == SENT).any())


@pytest.mark.parametrize("n,mix", um.POLYAK_CASES)
def test_polyak(n, mix):
    from sdreamer import kernels as K
    i = um.polyak_inputs(n)
    dst = _d(i["dst"]).clone()
    K.polyak(_d(i["src"]), dst, mix)
    got = {"dst": _h(dst)}
    # the existing figure: within 1 ulp of the float32 torch expression (two float32 evaluations, fma or not)
    f32 = (mix * i["src"] + (1 - mix) * i["dst"]).numpy()
    assert (np.abs(got["dst"].astype(np.float64) - f32) <= parity.ulp(f32)).all()
    if mix == 1.0:
        assert np.array_equal(got["dst"], i["src"].numpy())
    _check("polyak", got, um.reference("polyak", (n, mix)), f"n={n} mix={mix}")


# ------------------------------------------------------------------------------------------------ replay slices
def _slice_call(keys, B, t_idx, e_idx, scatter):
    """keys: (storage tensor, batch tensor, row bytes, steps, shift)"""
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    ks = nat.SliceKeys()
    for k, (sto, bat, rb, steps, shift) in enumerate(keys):
        ks.k[k].storage, ks.k[k].batch, ks.k[k].row_bytes = sto.data_ptr(), bat.data_ptr(), rb
        ks.k[k].steps, ks.k[k].shift = steps, shift
    ks.n = len(keys)
    starts = torch.tensor(um.SL_STARTS, dtype=torch.int64, device=DEV)
    pick = torch.tensor(um.SL_PICK, dtype=torch.int64, device=DEV)
    nat.call("sd_replay_slices", ctypes.addressof(ks), K.p(starts), K.p(pick), B, um.SL_L, um.SL_CAP, um.SL_E,
             K.p(t_idx), K.p(e_idx), scatter, K.stream())
    torch.cuda.synchronize()


def _based(arr, base):
    """a device copy of arr that starts `base` elements into its allocation"""
    t = torch.from_numpy(arr)
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device=DEV)
    v = buf[base:base + t.numel()].view(t.shape)
    v.copy_(t)
    return v, buf


def test_replay_slices_gather():
    sto = um.slice_storage()
    ref = um.ref_slices_gather()
    B = len(um.SL_PICK)
    keys, bats, holds = [], {}, []
    for name, dtype, w, steps, shift, base in um.SL_KEYS:
        v, buf = _based(sto[name], base)
        holds.append(buf)
        es = np.dtype(dtype).itemsize
        assert v.data_ptr() % 16 == (base * es) % 16
        bats[name] = torch.zeros(B, steps, w, dtype=v.dtype, device=DEV)
        assert bats[name].data_ptr() % 16 == 0
        keys.append((v, bats[name], w * es, steps, shift))
    t_idx = torch.full((B, um.SL_L), -1, dtype=torch.int64, device=DEV)
    e_idx = torch.full((B, um.SL_L), -1, dtype=torch.int64, device=DEV)
    _slice_call(keys, B, t_idx, e_idx, 0)
    for name in bats:
        assert np.array_equal(_h(bats[name]), ref[name]), name
    assert np.array_equal(_h(t_idx), ref["t_idx"]) and np.array_equal(_h(e_idx), ref["e_idx"])
    for (v, *_), (name, *_r) in zip(keys, um.SL_KEYS):  # the storage is read only
        assert np.array_equal(_h(v), sto[name]), name


@pytest.mark.parametrize("w", [4, 3])
def test_replay_slices_scatter(w):
    """w = 4: 16-byte rows (vector copies); w = 3: 12-byte rows (byte copies). Rows of two and three writers take the
    largest b; every row no slice covers keeps its bytes."""
    ref, cnt = um.ref_slices_scatter(w)
    assert {2, 3} <= set(cnt.ravel()) and (cnt == 0).any()
    B = len(um.SL_PICK)
    sto = torch.full((um.SL_CAP, um.SL_E, w), um.SL_SENT, device=DEV)
    bat = _d(um.slice_scatter_batch(w))
    _slice_call([(sto, bat, 4 * w, um.SL_L, 1)], B, None, None, 1)
    assert np.array_equal(_h(sto), ref)
    assert bool((sto[torch.from_numpy(cnt == 0).to(DEV)] == um.SL_SENT).all())


# ------------------------------------------------------------------------------------------------ refusals
def test_entry_points_refuse_what_they_cannot_run():
    """Every call below returns before any launch (SD_ESHAPE / SD_EARG -> NativeError), so none reaches the device;
    the buffers are real and large enough for the nearest admitted shape all the same."""
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    z = torch.zeros(4096, device=DEV)
    P, s = K.p(z), K.stream()

    def refused(name, *args):
        with pytest.raises(nat.NativeError):
            nat.call(name, *args)

    refused("sd_barlow_loss", P, 0, 5e-4, P, 256, P, s)  # E <= 0
    refused("sd_barlow_loss", P, -1, 5e-4, P, 256, P, s)
    refused("sd_barlow_loss", P, 4, 5e-4, P, 0, P, s)  # nblocks <= 0
    for nulls in ((0, P, P), (P, 0, P), (P, P, 0)):
        refused("sd_barlow_loss", nulls[0], 4, 5e-4, nulls[1], 256, nulls[2], s)
    refused("sd_standardize", P, P, P, P, 4, 0, 1e-8, s)  # C <= 0
    refused("sd_mask_rows", P, P, 1, P, 4, 0, s)  # width <= 0
    refused("sd_barlow_dc", P, P, P, 0, 5e-4, s)  # E <= 0
    for off in (-1, 2):  # label_off + n > ncol, as the forward
        refused("sd_infonce_fwd", P, 4, 3, 4, off, P, P, P, s)
        refused("sd_infonce_bwd", P, 4, 3, 4, off, P, P, 1.0, P, s)
    for r in (0, 1):  # one row has no unbiased std
        refused("sd_colstats", P, r, 4, P, P, s)
        refused("sd_standardize_bwd", P, P, P, P, P, r, 4, 1e-8, s)
    refused("sd_colstats", P, 4, 0, P, P, s)
    torch.cuda.synchronize()
    assert not z.any()
