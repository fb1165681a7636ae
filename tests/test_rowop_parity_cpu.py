"""CPU checks of tests/rowop_models.py, the case module behind tests/test_gpu_rowops_f64.py:

  * the arm functions restate the library's dispatch (cross-checked against its host-only sd_rmsnorm_bwd_blocks /
    sd_colsum_chunks) and the case tables reach every reachable arm; the unreachable RMSNorm arms are listed by name;
  * every input condition the GPU comparison relies on holds (index margins, rows on both sides of the free nats,
    |action| > 1, targets on and off the bins, ties, both sides of ReturnEMA's max(e1 - e0, 1));
  * the float32 restatement passes every comparison at every case using at most 1/8 of the tolerance (a third where
    8 x the measured error exceeds the existing cap and the cap is the tolerance);
  * a planted fault fails the comparison at every case where it can change the output, and reproduces the float32
    restatement bit for bit where it cannot.
"""
import numpy as np
import pytest
import torch

import rowop_models as rm

F32, F64 = torch.float32, torch.float64


def _cases(fam):
    cases = rm.FAMILIES[fam][0]
    if fam == "rms":
        return [(c, act) for c in cases for act in (0, 1)]
    return [(c, None) for c in cases]


def _run(fam, case, act, dt, fault=None):
    if fam == "rms":
        return rm.ref_rms(case, act, dt, fault)
    return rm.FAMILIES[fam][1](case, dt, fault)


def _name(case):
    return getattr(case, "name", str(case))


# ------------------------------------------------------------------------------------------------ arms
def test_arm_functions_match_the_library():
    from sdreamer import _native as nat
    for N in (1, 16, 17, 64, 65, 256, 1024, 1025, 4096):
        for M in (1, 3, 4, 5, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8195, 131075):
            assert rm.rms_bwd_blocks(M, N) == nat.fns["sd_rmsnorm_bwd_blocks"](M, N), (M, N)
    for R_ in (1, 511, 512, 513, 1024, 1025, 1029, 20000):
        assert rm.colsum_chunks(R_) == nat.fns["sd_colsum_chunks"](R_), R_


def test_unreachable_rms_arms_are_unreachable():
    seen = set()
    for N in range(1, 4097):
        seen.add(rm.rms_arm(N, aligned=False))
        seen.add(rm.rms_arm(N, aligned=True))
    assert seen == set(rm.RMS_ARMS_REACHABLE)
    assert not seen & set(rm.RMS_ARMS_UNREACHABLE)
    assert {(t, v) for t in (16, 64, 256) for v in (1, 2, 3, 4, 8, 16)} - seen == set(rm.RMS_ARMS_UNREACHABLE)


def test_rms_tables_reach_every_reachable_arm():
    fwd = {c.arms()[0] for c in rm.RMS_CASES}
    bwd = {c.arms()[1] for c in rm.RMS_CASES if c.bwd}
    assert fwd == set(rm.RMS_ARMS_REACHABLE) and bwd == set(rm.RMS_ARMS_REACHABLE)
    # the 256-wide row outside the vector form: the scalar team-64 arm at VPT 4, by ld and by alignment
    assert rm.RMS["5x256-ld4"].arms() == (("vec", 1), ("vec", 1))
    assert rm.RMS["5x256-ld1"].arms() == ((64, 4), (64, 4))
    assert rm.RMS["5x256-mis"].arms() == ((64, 4), (64, 4))
    assert rm.RMS["5x256-dymis"].arms() == (("vec", 1), (64, 4))
    # grid-stride loops: a block owns rows of more than one stride, in every kind of kernel
    kinds = lambda cs: {("vec" if c.arms()[0][0] == "vec" else c.arms()[0][0]) for c in cs}  # noqa: E731
    stride_b = [c for c in rm.RMS_CASES if c.bwd and c.M > rm.rms_bwd_blocks(c.M, c.N) * rm.rms_rows_per_block(c.N)]
    stride_f = [c for c in rm.RMS_CASES if c.M > 8192 * rm.rms_rows_per_block(c.N)]
    assert kinds(stride_b) == {16, 64, 256, "vec"} and kinds(stride_f) == {16, 64, 256, "vec"}
    assert all(rm.rms_bwd_blocks(c.M, c.N) == 512 for c in stride_b)
    assert all(not c.bwd and rm.rms_fwd_blocks(c.M, c.N) == 8192 for c in stride_f)
    assert max(c.M * c.N * 4 for c in rm.RMS_CASES) < 35e6
    # flags
    for n in (65, 256):
        flagged = [c for c in rm.RMS_CASES if (c.M, c.N) == (5, n)]
        assert any(c.acc_dx for c in flagged) and {c.dw for c in flagged} == {"acc", "set", None}
        assert any(c.eps == rm.EPS32 for c in flagged) and any(c.zero_row for c in flagged)


def test_other_tables_reach_every_arm():
    arms = {(c.arm(), c.R > rm.COLSUM_RCH) for c in rm.COLSUM_CASES}
    assert arms == {("short", False), ("kernel", False), ("kernel", True), ("two_pass", True)}
    assert rm.COLSUM["512x4096"].arm() == "short" and rm.COLSUM["512x4097"].arm() == "kernel"
    assert any(c.ld and c.ld > c.N for c in rm.COLSUM_CASES)
    assert {c.accumulate for c in rm.COLSUM_CASES} == {True, False}
    assert {rm.team(c.K) for c in rm.TEAM_CASES} == {8, 16, 32, 64}
    for T in (8, 16, 32, 64):  # a full team, a partly filled one, and a partly filled last block
        ks = {c.K for c in rm.TEAM_CASES if rm.team(c.K) == T}
        assert T in ks and any(k < T for k in ks)
    assert all(any((c.groups * rm.team(c.K)) % 256 for c in rm.TEAM_CASES if c.K == K) for K in rm.TEAM_KS)
    assert {rm.team(c.K) for c in rm.KL_CASES} == {8, 16, 32, 64}
    assert any(c.rows > 4096 for c in rm.KL_CASES)  # the grid-stride loop of kl_fwd
    assert any(c.S % (256 // rm.team(c.K)) for c in rm.KL_CASES) and any(c.K < rm.team(c.K) for c in rm.KL_CASES)
    assert {(c.arm(), c.form) for c in rm.LRET_CASES} >= {("staged", "replay"), ("staged", "imag"),
                                                         ("unstaged", "replay"), ("unstaged", "imag"),
                                                         ("unstaged", "both")}
    assert rm.LRET["N17-T255-replay"].arm() == "staged" and rm.LRET["N17-T256-replay"].arm() == "unstaged"
    assert 4 * 16 * 255 * 4 == 65280  # the staged kernel's dynamic LDS at its limit
    assert {rm.ema_arm(c.n) for c in rm.EMA_CASES} == {"regs", "global"}
    assert rm.ema_arm(16384) == "regs" and rm.ema_arm(16385) == "global"
    assert {c.NB for c in rm.TWOHOT_CASES} == {1, 3, 63, 65, 129, 255, 256}
    assert any(c.Tr == c.Tl for c in rm.REPVAL_CASES) and any(c.Tr < c.Tl - 1 for c in rm.REPVAL_CASES)
    assert any(c.H1 > c.H + 1 for c in rm.IMAG_AC_CASES)


# ------------------------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("name", [c.name for c in rm.TEAM_CASES])
def test_sampler_margins(name):
    c = rm.TEAMC[name]
    r32, r64 = rm.ref_sample(c, F32), rm.ref_sample(c, F64)
    assert min(r32["@margin"], r64["@margin"]) >= rm.MIN_MARGIN, (r32["@margin"], r64["@margin"])
    assert np.array_equal(r32["index"], r64["index"])


@pytest.mark.parametrize("name", [c.name for c in rm.KL_CASES])
def test_kl_rows_on_both_sides_of_free(name):
    c = rm.KL[name]
    kl, free = rm.ref_kl(c)["kl"], rm.kl_inputs(c)["free"]
    assert np.abs(kl - free).min() >= rm.KL_FREE_GAP
    if c.K > 1:  # one category: KL = 0 in every row, all below
        assert (kl < free).any() and (kl > free).any()
    else:
        assert (kl == 0).all() and free > 0


def test_head_inputs():
    for c in rm.BN_CASES:
        assert rm.bn_inputs(c)["action"].abs().max() > 1
    for c in rm.TWOHOT_CASES + rm.REPVAL_CASES:
        i = rm.twohot_inputs(c) if isinstance(c, rm.TwohotCase) else rm.repval_inputs(c)
        bins = i["bins"]
        assert len(bins) == c.NB and (c.NB == 1 or bool((bins[1:] >= bins[:-1]).all()))
    for c in rm.TWOHOT_CASES:
        if c.rows < 5 or c.NB < 3:
            continue
        i = rm.twohot_inputs(c)
        t, bins = i["target"], i["bins"]
        on = [bool((bins == v).any()) for v in t[:5]]
        assert on == [False, True, False, False, True]  # between, on a bin, -1e9, +1e9, 0.0 (a bin)
        assert bins[0] < t[0] < bins[-1] and t[2] < bins[0] and t[3] > bins[-1] and t[4] == 0
    for c in rm.REPVAL_CASES:
        la = rm.repval_inputs(c)["last"][:, :c.Tr]
        assert c.B == 1 or (bool((la == 1).any()) and bool((la == 0).any()))
    i = rm.bern_inputs(257)
    assert i["logit"].min() == -40 and i["logit"].max() == 40
    for c in rm.LRET_CASES:
        if c.form != "imag" and c.T >= 2:
            i = rm.lret_inputs(c)
            la, te = i["last"][:, 1:], i["term"][:, 1:]
            assert bool((la == 1).any())
            if c.N >= 3:
                assert bool(((la == 1) & (te == 0)).any() and ((la == 0) & (te == 1)).any()
                            and ((la == 1) & (te == 1)).any())


def test_ema_inputs():
    scale_clamped, scale_free = 0, 0
    for c in rm.EMA_CASES:
        i, r = rm.ema_inputs(c), rm.ref_ema(c)
        x = i["x1"]
        if c.kind == "constant":
            assert x.unique().numel() == 1
        if c.kind == "two_values" and c.n >= 21:
            assert x.unique().numel() == 2
        if c.kind == "ties" and c.n >= 1000:
            assert x.unique().numel() < c.n // 4
        if c.kind == "zeros_mix" and c.n >= 21:
            assert bool((x == 0).any()) and bool(torch.signbit(x[x == 0]).any()) and bool((x < 0).any())
        for k in ("1", "2"):
            e = r["ema" + k]
            scale_clamped += e[1] - e[0] < 1
            scale_free += e[1] - e[0] > 1
            assert abs(e[1] - e[0] - 1) > 1e-4
    assert scale_clamped and scale_free
    spread = {c.kind: np.diff(rm.ref_ema(c)["q1"])[0] for c in rm.EMA_CASES if c.n == 1000}
    assert spread["constant"] < 1 < spread["normal10"]


# ------------------------------------------------------------------------------------------------ the comparison
@pytest.mark.parametrize("fam", list(rm.FAMILIES))
def test_float32_restatement_passes_with_room(fam):
    worst = {}
    for case, act in _cases(fam):
        ref = rm.reference(fam, case, act)
        got = _run(fam, case, act, F32)
        rm.compare(fam, got, ref, f"{fam} {_name(case)}")
        for k, (a, b) in rm.ratios(fam, got, ref).items():
            worst[k] = max(worst.get(k, (0, 0)), (a, b, _name(case)))
    print(fam, {k: f"{a:.3g} of the bound, {b:.3g} of the cap ({n})" for k, (a, b, n) in worst.items()})
    # 1/8 of the tolerance; a third where the tolerance is the cap itself (rowop_models.Tol.capped)
    room = {k: 1 / 3 if rm.TOL[fam][k].capped else 0.125 for k in worst}
    assert all(a <= room[k] and b <= room[k] for k, (a, b, _) in worst.items()), worst


@pytest.mark.parametrize("fam,fault", [(f, x) for f, xs in rm.FAULTS.items() for x in xs])
def test_planted_fault_fails(fam, fault):
    caught, same = [], []
    for case, act in _cases(fam):
        ref = rm.reference(fam, case, act)
        base = _run(fam, case, act, F32)
        bad = _run(fam, case, act, F32, fault)
        if rm.same_bits(base, bad):
            same.append(_name(case))
            continue
        assert not rm.passes(fam, bad, ref), f"{fault} changes {fam} {_name(case)} and is not caught"
        caught.append(_name(case))
    print(fam, fault, "caught at", len(caught), "cases; cannot change", len(same), same[:12])
    assert caught
