"""CPU checks of tests/gemm_models.py, the case module behind tests/test_gpu_gemm_f64.py:

  * the case tables reach every arm the restated dispatch (f32_arm, bf16x3_arm, mlp_arm) can return, the arms no entry
    point reaches are listed by name, and kernels._layout reads every view as the layout the case names;
  * the case conditions hold: guard bands large enough, no sum of |terms| is 0 where a bound is relative to it, every
    stated tail and empty split is there;
  * g3_tile's and gemm3_w256_kernel's workgroup remaps are bijections for every tile count 1 .. 64 and at each case;
  * the float32 restatement and the split model pass their bounds with room;
  * every planted fault fails wherever it changes a bit, and reproduces the unfaulted evaluation elsewhere;
  * kernels._skinny_split, _auto_split and _fast_split return a split in [1, 64] at every table shape.
"""
import itertools

import pytest
import torch

import gemm_models as gm

F32, F64 = gm.F32, gm.F64
SMALL = 1 << 20  # planted faults run on the cases with at most this many outputs (the rest repeat their arms)


def _arms(fam):
    for c in gm.CASES[fam]:
        yield c, gm.arm_of(c, gm.gemm_inputs(c).d)


@pytest.fixture(scope="module")
def arms():
    return {fam: list(_arms(fam)) for fam in ("f32", "bf16x3", "wgrad")}


# ------------------------------------------------------------------------------------------------ arms
# Arms the kernels instantiate that no call through their entry point reaches:
UNREACHABLE = {
    "gemm_m16 / gemm_skinny <BKC = false, VB = true>": "launch_m16 / launch_skinny fold VB into BKC && VB",
    "gemm_m16 / gemm_skinny with the capped reduce": "sd_gemm_f32 passes cap = false on the skinny route",
    "f32 tile 3 chosen automatically": "the automatic choice returns 0, 1 or 2",
    "split-bf16 tile 2 chosen automatically": "gemm3_run's automatic choice returns 0 or 1 (retired, see its comment)",
    "gemm3_kernel <AK = true, RS = true>": "the entries that pass a rowsum refuse a k-contiguous A",
    "gemm3_w256_kernel with an input norm": "the wide route is taken only when no norm weight is set",
    "sd_gemm_bf16x3_wgrad* at batch > 1": "refused (SD_ESHAPE): the row sums' partials have no batch index",
}


def test_f32_tables_reach_every_arm(arms):
    seen = {(a.kernel, a.AK, a.BKC, a.VA, a.VB, a.reduce) for _, a in arms["f32"]}
    want = set()
    for k in ("m16", "skinny"):
        want |= {(k, True, bkc, va, vb, red) for bkc, va, vb, red in itertools.product((True, False), repeat=4)
                 if bkc or not vb}
    for t in range(4):
        want |= {(f"tile{t}", ak, bkc, va, vb, red) for ak, bkc, va, vb, red in itertools.product((True, False), repeat=5)}
    assert want <= seen, sorted(want - seen)
    assert not any(a.kernel in ("m16", "skinny") and not a.BKC and a.VB for _, a in arms["f32"])
    byname = {c.name: a for c, a in arms["f32"]}
    auto = {(c.M, c.N, c.K, c.batch): a.kernel for c, a in arms["f32"] if c.group == "auto"}
    assert auto == {(33, 1, 1, 256): "tile0", (33, 1, 1, 1): "tile1", (20, 40, 50, 1): "tile2"}
    assert [a.capped for c, a in arms["f32"] if c.group == "capped"] == [True]
    assert sum(a.capped for a in byname.values()) == 1
    assert {a.kernel for c, a in arms["f32"] if c.group == "k0"} >= {"m16", "tile2"}
    assert all(a.ks == 1 for c, a in arms["f32"] if c.K == 0)
    for k in ("m16", "skinny", "tile1"):  # beta = 0 over NaN, split and unsplit
        assert {a.reduce for c, a in arms["f32"] if c.nanc and a.kernel == k} == {True, False}, k
    assert any(c.padc and c.alpha == 0.5 and c.beta == 1.0 for c, _ in arms["f32"])
    assert any(c.bias == 2 and c.batch > 1 and a.kernel == k for c, a in arms["f32"] for k in ("m16",))
    assert any(c.bias == 2 and c.batch > 1 and a.kernel == "skinny" for c, a in arms["f32"])


def test_split_bf16_tables_reach_every_arm(arms):
    g3 = [(c, a) for c, a in arms["bf16x3"] if not getattr(a, "fallback", False)]
    seen = {(a.kernel, a.AK, a.BKC, a.VA, a.VB) for _, a in g3}
    want = {(f"g3tile{t}", ak, bkc, va, vb) for t in (0, 1) for ak, bkc, va, vb in itertools.product((True, False), repeat=4)}
    assert want <= seen, sorted(want - seen)
    assert ("g3tile2", False, False, True, True) in seen
    assert {a.fallback for c, a in arms["bf16x3"] if c.group == "fallback"} == {True}
    assert {(c.M, c.N, c.K) for c, a in arms["bf16x3"] if c.group == "fallback"} == {(63, 64, 64), (64, 63, 64), (64, 64, 63)}
    assert any(a.asked == 2 and a.kernel == "g3tile0" for _, a in g3)  # the downgrade
    assert any(c.tile == -1 and c.batch == 192 and a.kernel == "g3tile0" for c, a in g3)
    assert any(c.tile == -1 and a.kernel == "g3tile1" for c, a in g3)
    assert {(a.order, a.ks > 1) for c, a in g3 if c.bcast} == {("bcastA", False), ("plain", True)}
    counts = {a.grid[0] * a.grid[1] * a.grid[2] for c, a in g3}
    assert {3, 8, 15, 193} <= counts
    bc = {a.grid[0] * a.grid[1] * a.grid[2] for c, a in g3 if a.order == "bcastA"}
    assert any(t < 8 for t in bc) and any(t % 8 for t in bc if t > 8) and any(t % 8 == 0 for t in bc)
    assert any(not a.VA and not a.VB and c.va == "stride" for c, a in g3)
    assert any(not a.VA and c.va == "off" for c, a in g3) and any(not a.VB and c.vb == "off" for c, a in g3)
    assert {a.reduce for _, a in g3} == {True, False}
    wg = arms["wgrad"]
    assert all(a.RS for _, a in wg)
    want = {(f"g3tile{t}", bkc, red, acc, al) for t in (0, 1) for bkc in (True, False) for red in (True, False)
            for acc in (0, 1) for al in (1.0, 0.5)}
    want |= {("g3tile2", False, red, acc, al) for red in (True, False) for acc in (0, 1) for al in (1.0, 0.5)}
    seen = {(a.kernel, a.BKC, a.reduce, c.acc, c.alpha) for c, a in wg}
    assert want <= seen, sorted(want - seen)
    assert {c.rs_split for c, _ in wg if c.entry == "wgrad2"} >= {1, 64, 65, 256}
    assert all(c.M == 257 for c, _ in wg if c.rs_split == 256)
    assert {c.M for c, _ in wg} == {64, 65, 257, 130} and {c.K for c, _ in wg} >= {64, 96, 100}


def test_mlp_tables_reach_every_arm():
    seen = {gm.mlp_arm(gm.mlp_desc(c)) for c in gm.MLP_CASES}
    assert seen == ({("mlp128", r, p) for r in (True, False) for p in (True, False)}
                    | {("w256", False, True), ("w256", False, False)})
    po = [c for c in gm.MLP_CASES if c.pout]
    assert {c.N for c in po} >= {64, 128, 192, 256, 320} and {c.N for c in gm.MLP_CASES if not c.pout} >= {65, 255}
    assert {c.M for c in gm.MLP_CASES} >= {1, 127, 129, 257, 12033} and {c.K for c in gm.MLP_CASES} == {32, 64, 96}
    assert {c.npin for c in gm.MLP_CASES if c.rms} == {1, 3} and {c.act for c in gm.MLP_CASES if c.rms} == {0, 1}
    assert {c.batch for c in gm.MLP_CASES if not c.rows} >= {1, 3, 5, 192}
    ent = [c for c in gm.MLP_CASES if c.rows]
    assert any(set(c.rows) >= {1, 64, c.N} for c in ent) and any(c.null >= 0 and c.rms for c in ent)
    assert any(c.null >= 0 and not c.rms for c in ent) and any(c.bcast for c in gm.MLP_CASES)
    odd = [c for c in gm.MLP_CASES if c.pout and (c.N // 64) % 2 and c.batch > 1]
    assert {(c.N, bool(c.rows)) for c in odd} >= {(n, f) for n in (64, 192, 320) for f in (True, False)}
    wide = [c for c in gm.MLP_CASES if gm.mlp_arm(gm.mlp_desc(c))[0] == "w256"]
    assert {(c.M, c.K, c.pout) for c in wide if c.batch == 192} == set(itertools.product((1, 257), (32, 64, 96), (False, True)))
    assert any(c.M == 12033 and c.rows and gm.cdiv(c.M, 256) == 48 and c.M % 256 == 1 for c in wide)
    assert {c.K // 32 for c in wide} == {1, 2, 3}  # gemm3_w256_kernel's clamped prefetch: one, two and three k tiles
    assert max(c.batch * c.M * c.N * 4 for c in gm.MLP_CASES) < 52e6


def _mlp_override(r):
    what, val = r.change
    c = r.base
    if what == "null":
        return {"x": False} if val == "x" else None
    if what == "dim":
        k, v = val
        key = {"a_kcontig": "ak", "b_kcontig": "bk", "strideB": "sB"}.get(k, k)
        return {key: v}
    if what == "ext":
        return {val[0]: val[1]}
    f, b, v = val
    if f == "norm_w_ptr":
        return {"norm_w_ptr": tuple(x and i != b for i, x in enumerate(gm.mlp_desc(c).norm_w_ptr))}
    if f == "w_rows":
        return {"w_rows": tuple(v if i == b else x for i, x in enumerate(gm.mlp_desc(c).w_rows))}
    return {"w_ptr_aligned": False}


def test_refusals_follow_the_restated_dispatch():
    codes = set()
    for r in gm.REFUSALS:
        what, val = r.change
        if r.entry == "mlp":
            over = _mlp_override(r)
            if over is None:
                continue  # a null pointer of the descriptor: the entry's first line
            assert gm.mlp_arm(gm.mlp_desc(r.base, **over)) == r.expect, r.name
        elif what in ("tile", "dim", "rs_split"):
            d = gm.gemm_inputs(r.base).d
            rs = r.base.rs_split if r.entry == "wgrad2" else None
            if what == "tile":
                d.tile = val
            elif what == "rs_split":
                rs = val
            else:
                setattr(d, {"a_kcontig": "ak"}.get(val[0], val[0]), val[1])
            a = gm.f32_arm(d) if r.entry == "f32" else gm.bf16x3_arm(d, r.entry.startswith("wgrad"), rs)
            assert a == r.expect, r.name
        codes.add((r.entry, r.expect))
    assert codes >= {(e, gm.SD_EARG) for e in ("f32", "bf16x3", "wgrad", "wgrad2", "mlp")}
    assert codes >= {(e, gm.SD_ESHAPE) for e in ("wgrad", "wgrad2", "mlp")}
    assert len({r.name for r in gm.REFUSALS}) == len(gm.REFUSALS)
    assert gm.mlp_arm(gm.mlp_desc(gm._RM)) == ("mlp128", True, True)


def test_views_are_the_layouts_the_cases_name():
    from sdreamer import kernels
    for fam in ("f32", "bf16x3", "wgrad"):
        for c in gm.CASES[fam]:
            if c.K == 0:
                continue
            inp = gm.gemm_inputs(c)
            a, b = inp.bufA.view(inp.bufA.host), inp.bufB.view(inp.bufB.host).transpose(1, 2)
            if c.batch == 1:
                la, lb = kernels._layout(a[0], 0, 1), kernels._layout(b[0], 1, 0)
            else:
                la, lb = kernels._layout(a, 1, 2), kernels._layout(b, 2, 1)
            assert la == (c.ak, inp.d.lda) and lb == (c.bk, inp.d.ldb), (c.name, la, lb)
            assert torch.equal(a, inp.A.expand(c.batch, c.M, c.K)) and torch.equal(b.transpose(1, 2), inp.B)
    assert kernels._fast_split(130, 64, 1100, 1) == 2  # the split the kernels.wgrad / wgrad2 cases are evaluated at
    assert [c.ksplit for c in gm.WGRAD_CASES if c.group == "wgrad-py"] == [2, 2]


# ------------------------------------------------------------------------------------------------ case conditions
def test_case_conditions(arms):
    for fam in ("f32", "bf16x3", "wgrad"):
        for c, a in arms[fam]:
            inp = gm.gemm_inputs(c)
            for buf in (inp.bufA, inp.bufB, inp.bufC, inp.bufBias, inp.bufRs, inp.bufRs2, inp.bufWs):
                if buf is not None:
                    assert buf.start >= gm.GUARD and buf.n - buf.start - buf.ext >= gm.GUARD and gm.GUARD % 4 == 0
            assert inp.bufWs.ext == gm.ws_floats(c)
            assert (gm.evaluate(c, inp)["C@scale"] > 0).all(), c.name
            if c.entry.startswith("wgrad"):
                assert (gm.evaluate(c, inp)["rowsum@scale"] > 0).all()
            assert c.K == 0 or a.VA == (c.va in ("v", "pad") or c.va == "stride" and c.batch == 1), c.name
    empty = [(c, a) for fam in arms for c, a in arms[fam] if a.ks > 1 and (a.ks - 1) * a.kchunk >= c.K > 0]
    assert {a.kernel for _, a in empty} >= {"m16", "skinny", "g3tile1"}
    assert any(c.K == 40 and a.ks == 4 and a.kchunk == 16 for c, a in empty)
    assert any(c.K == 64 and a.ks == 3 and a.kchunk == 32 and a.kernel.startswith("g3") for c, a in empty)
    for k, sweep in (("m16", 512), ("skinny", 128)):
        ks = {c.K for c, a in arms["f32"] if a.kernel == k}
        assert any(0 < x < sweep for x in ks) and sweep in ks and sweep + 1 in ks and any(x > 2 * sweep for x in ks)
    assert any(c.K % 4 and a.kernel.startswith("tile") for c, a in arms["f32"])
    for c in gm.MLP_CASES:
        if c.batch * c.M * c.N > SMALL:
            continue
        inp = gm.mlp_inputs(c)
        ref = gm.evaluate(c, inp)
        rows = gm.mlp_rows(c)
        for b, r in enumerate(rows):
            assert (ref["C@scale"][b, :, :r] > 0).all() and not ref["C"][b, :, r:].any()
        if c.pout:
            assert inp.bufPout.n - inp.bufPout.start - inp.bufPout.ext >= gm.GUARD + c.M
            full = [q for q in range(c.N // 64) if all(64 * q < r for r in rows)]
            assert (ref["pout@sq"][:, full] > 0).all()
        if c.rms:
            assert (inp.pin > 0).all()


# ------------------------------------------------------------------------------------------------ the remaps
@pytest.mark.parametrize("fault", [None, "remap_rem"])
def test_remaps_are_bijections(arms, fault):
    bad = []
    grids = [(nx, T // nx, 1) for T in range(1, 65) for nx in (1, 2, 3, 5) if T % nx == 0]
    grids += [(1, 1, T) for T in range(1, 65)] + [(2, 3, T) for T in (3, 4)]
    grids += [a.grid for fam in ("bf16x3", "wgrad") for _, a in arms[fam] if hasattr(a, "grid")]
    grids += [(gm.cdiv(c.N, 128), gm.cdiv(c.M, 128), c.batch) for c in gm.MLP_CASES]
    for nx, ny, nz in set(grids):
        T = nx * ny * nz
        for bcast in (False, True):
            cells = [gm.g3_remap(L, nx, ny, nz, bcast, fault) for L in range(T)]
            if not gm.is_bijection(cells, list(itertools.product(range(nx), range(ny), range(nz)))):
                bad.append(("g3", nx, ny, nz, bcast))
    wide = [(gm.cdiv(c.M, 256), c.batch) for c in gm.MLP_CASES if c.N == 256 and not c.rms]
    for rt, batch in set(wide) | {(T, 1) for T in range(1, 65)} | {(T, 4) for T in range(1, 17)}:
        cells = [gm.w256_remap(L, rt * batch, batch, fault) for L in range(rt * batch)]
        if not gm.is_bijection(cells, list(itertools.product(range(batch), range(rt)))):
            bad.append(("w256", rt, batch))
    if fault is None:
        assert not bad, bad[:10]
    else:  # the off-by-one in rem: both remaps stop being bijections
        assert {b[0] for b in bad} == {"g3", "w256"}


# ------------------------------------------------------------------------------------------------ the comparison
def _evals(c, fault=None):
    """(family the comparison runs in, what a correct float32 evaluation gives, reference, split model, arm)"""
    fam = gm.family(c)
    inp = gm.inputs(c)
    arm = None if fam == "mlp" else gm.arm_of(c, inp.d)
    fam_c = "f32" if gm.routed_f32(c, arm) else fam
    ref = gm.evaluate(c, inp)
    split = gm.evaluate(c, inp, "split", F64) if fam_c != "f32" else None
    kind = "plain" if fam_c == "f32" else "split"
    base = gm.evaluate(c, inp, kind, F32)
    bad = gm.evaluate(c, inp, kind, F32, fault) if fault else None
    return fam, fam_c, base, bad, ref, split, arm


@pytest.mark.parametrize("fam", list(gm.CASES))
def test_restatement_passes_with_room(fam):
    worst = {}
    for c in gm.CASES[fam]:
        _, fam_c, got, _, ref, split, arm = _evals(c)
        if "pout" in got:
            got["pout_own"] = gm.own_pout(got["C"])
        assert not gm.failures(fam, got, ref, split, arm), c.name
        for k, v in gm.units(fam_c, got, ref, split).items():
            key = (fam_c, "rowsum" if k == "rowsum2" else k)
            worst[key] = max(worst.get(key, (0.0, "")), (v, c.name))
    print(fam, {f"{f}.{k}": (round(v, 3), n) for (f, k), (v, n) in worst.items()})
    for (f, k), (v, n) in worst.items():
        t = gm.TOL[f][k]
        room = 1 / 3 if t.k >= t.cap else 0.125
        assert v <= room * t.k, (f, k, v, n)


@pytest.mark.parametrize("fam,fault", [(f, x) for f, xs in gm.FAULTS.items() for x in xs])
def test_planted_fault_fails(fam, fault):
    caught, same = [], []
    for c in gm.CASES[fam]:
        if c.batch * c.M * c.N > SMALL:
            continue
        _, fam_c, base, bad, ref, split, arm = _evals(c, fault)
        if gm.same_bits(base, bad):
            same.append(c.name)
            continue
        assert gm.failures(fam, bad, ref, split, arm), f"{fault} changes {c.name} and is not caught"
        caught.append(c.name)
    print(fam, fault, "caught at", len(caught), "cases; cannot change", len(same))
    assert caught


def test_every_named_fault_is_planted():
    planted = {x for xs in gm.FAULTS.values() for x in xs} | {"remap_rem"}
    assert planted == set(gm.GEMM_FAULTS + gm.SPLIT_FAULTS + gm.RS_FAULTS + gm.MLP_FAULTS) | {"remap_rem"}
    assert len(planted) == 14


def test_python_split_choices_stay_in_range():
    from sdreamer import kernels
    shapes = {(c.M, c.N, c.K, c.batch) for fam in gm.CASES for c in gm.CASES[fam]}
    for M, N, K, b in shapes:
        for f in (kernels._skinny_split, kernels._auto_split, kernels._fast_split):
            assert 1 <= f(M, N, K, b) <= 64, (f.__name__, M, N, K, b)
