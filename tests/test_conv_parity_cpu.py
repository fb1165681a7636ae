"""CPU self-check of the conv stage parity tests (tests/conv_models.py; tests/test_gpu_conv_f64.py runs the same cases
and comparisons on the product). For every case:

1. the tie margin that lets the GPU test demand an equal argmax at every pooling window: the smallest top-2 margin of
   the float64 conv output over all windows is >= 32 x the case's worst float32-restatement conv-output error
   (measured here, not a constant), and the float32 restatement picks the same argmax everywhere. A case that misses
   it gets another seed in conv_models.py (the first of 0 .. 15 that meets it);
2. the comparison functions pass the float32 restatement against float64;
3. they fail on deliberately wrong float64 references: the pad's two sides swapped (even kernels) or the right-most tap
   column blind to the image's last column (odd kernels); the last pooled column's gradient routed to window position
   0; the rows of dW at or above 16 floor(Co / 16) zeroed; the conv gradient's row / column that an odd size's pool
   dropped nonzero; the upsample reading min(xx, W - 1). Where a mutant cannot change a case the test asserts that it
   EQUALS the reference there, so the exception is checked, not skipped;
4. the Python restatement of the four host plans agrees with the library's host-only queries (nothing is launched)
   at every case and over a sweep of shapes.
"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_models as cm
from oracle import ref_cpu

F32, F64 = cm.F32, cm.F64
STAGE_IDS = [c.name for c in cm.STAGE_CASES]
UP_IDS = [c.name for c in cm.UP_CASES]
KERNEL_IDS = [c.name for c in cm.KERNEL_CASES]


def _native():
    try:
        from sdreamer import _native as nat
    except ImportError:
        pytest.skip("libsdhip.so is not built")
    return nat


# --------------------------------------------------------------------------------------------------- the reference
def test_reference_restates_the_oracle_conv_and_upsample():
    g = torch.Generator().manual_seed(5)
    for k in (3, 4, 5):
        x, w, b = (torch.randn(s, generator=g, dtype=F64) for s in ((2, 3, 5, 6), (4, 3, k, k), (4,)))
        assert torch.equal(cm.conv_same(x, w, b), ref_cpu.conv_same(x, w, b))
        assert torch.equal(cm.upsample2(x), F.interpolate(x, scale_factor=2, mode="nearest"))
        rms = F.rms_norm(x.permute(0, 2, 3, 1), (3,), b[:3], cm.EPS).permute(0, 3, 1, 2)
        assert torch.equal(rms, ref_cpu.rms2d(x, b[:3]))
    assert cm.EPS == 1e-4


# --------------------------------------------------------------------------------------------------- the cases
def test_case_tables_name_the_arms_the_plans_give():
    for c in cm.STAGE_CASES:
        assert cm.stage_arms(c) == (c.fwd, c.wgrad, c.dgrad), (c.name, cm.stage_arms(c))
    for c in cm.UP_CASES:
        assert cm.up_arms(c) == (c.fwd, c.wgrad, c.dgrad), (c.name, cm.up_arms(c))
    for c in cm.KERNEL_CASES:
        assert cm.kernel_arms(c) == (c.arm, c.fast), (c.name, cm.kernel_arms(c))


def test_case_tables_reach_every_arm():
    fwd = {c.fwd for c in cm.STAGE_CASES + cm.UP_CASES} | {c.arm for c in cm.KERNEL_CASES if c.op != "wgrad"}
    for arm in ["conv_fwd6r_direct_pool", "conv_fwd_direct_pool_c4", "conv_fwd16_pool<16>", "conv_fwd16_pool<32>",
                "conv_fwd16_pool<64>", "conv_fwd16<16>", "conv_fwd16<32>", "conv_fwd16<48>",
                "conv_fwd16<32> + pool_rms", "conv_fwd16<64> + pool_rms",
                "conv_fwd_kernel<128,32,VA,VB>", "conv_fwd_kernel<128,64,VA,VB>", "conv_fwd_kernel<128,32,VB>",
                "conv_fwd_kernel<128,64>", "conv_fwd_kernel<128,32,VA,VB> + pool_rms",
                "conv_fwd_kernel<128,64,VA,VB> + pool_rms"]:
        assert arm in fwd, arm
    wg = {c.wgrad.split(" ")[0] for c in cm.STAGE_CASES + cm.UP_CASES}
    wg |= {a.split(" ")[0] for c in cm.KERNEL_CASES if c.op == "wgrad" for a in (c.arm, c.fast) if a}
    want = [f"conv_wgrad_direct<{tm},{nbw}>" for tm, nbw in ((2, 2), (3, 4), (4, 7), (1, 10), (3, 10), (2, 4))]
    want += ["conv_wgrad_direct<1,7,WS>", "conv_wgrad_direct<2,7,WS>", "conv_wgrad_direct<2,7,WS,PL>",
             "conv_wgrad3_direct<1,7,WS,PL>", "conv_wgrad3_direct<2,7,WS,PL>"]
    want += [f"conv_wgrad3_direct<{tm},{nbw}>" for tm, nbw in ((2, 2), (2, 4), (3, 5), (3, 7), (4, 4), (1, 5), (3, 4))]
    want += ["conv_wgrad_kernel<64,64,VA,VB>", "conv_wgrad_kernel<32,128,VA,VB>", "conv_wgrad_kernel<32,128,VB>",
             "conv_wgrad_kernel<32,128,VA>", "conv_wgrad_kernel<32,128>"]
    for arm in want:
        assert arm in wg, arm
    assert any("gx=" in c.wgrad for c in cm.STAGE_CASES) and any("gx=" in c.arm for c in cm.KERNEL_CASES)
    dg = {c.dgrad for c in cm.STAGE_CASES + cm.UP_CASES} | {c.fast for c in cm.KERNEL_CASES if c.op == "dgrad"}
    for arm in ["conv_dgrad_pool_k", "conv_dgrad3_direct", "conv_dgrad3<16>", "conv_dgrad3<48>", "conv_dgrad3<64>",
                "conv_fwd_kernel<128,32,VA,VB>", "conv_fwd_kernel<128,64,VA,VB>", "conv_fwd_kernel<128,32>"]:
        assert arm in dg, arm
    # the shapes the suite never ran: even and 3 x 3 kernels, odd / non-square / tiny images, FiLM at ipc 2 and Nb
    S = cm.STAGE_CASES
    assert {3, 4, 5} <= {c.k for c in S}
    assert any(c.H % 2 and c.W % 2 for c in S) and any(c.H % 2 and not c.W % 2 for c in S)
    assert any(c.H > c.W for c in S) and any(c.H < c.W for c in S) and {2, 4} <= {c.W for c in S}
    assert any(c.ipc == 2 for c in S) and any(c.ipc == c.nb for c in S if c.ipc)
    assert any(c.co > 64 and c.k * c.k * c.ci // 4 > cm.MAX_TAPQ for c in S)


def test_reference_runs_leave_the_cached_inputs_alone():
    c = cm.STAGE["film_hw7"]
    cm.run_stage_ref(c, F32, "route"), cm.run_up_ref(cm.UP["up_k4"], F32, "ups")
    assert not any(t.requires_grad for t in cm.stage_inputs(c) + cm.up_inputs(cm.UP["up_k4"]))


# --------------------------------------------------------------------------------------------------- the tie margin
def _conv_err(c):
    return float(np.abs(cm.run_stage_ref(c, F32)["conv"] - cm.run_stage_ref(c, F64)["conv"]).max())


@pytest.mark.parametrize("name", STAGE_IDS)
def test_stage_inputs_have_no_near_ties(name):
    c = cm.STAGE[name]
    r32, r64 = cm.run_stage_ref(c, F32), cm.run_stage_ref(c, F64)
    err = _conv_err(c)
    print(f"{name}: smallest window margin {r64['margin']:.3g}, float32 conv error {err:.3g}")
    assert r64["margin"] >= cm.MARGIN_FACTOR * err, f"{name}: margin {r64['margin']:.3g} < 32 x {err:.3g}: another seed"
    assert np.array_equal(r32["amax"], r64["amax"])
    # the seed is the first that meets the margin (chosen from the reference alone), and one exists within 16 tries
    assert c.seed < cm.MAX_SEEDS
    for s in range(c.seed):
        e = cm.with_seed(c, s)
        margin = cm.run_stage_ref(e, F64)["margin"]
        assert margin < cm.MARGIN_FACTOR * _conv_err(e), f"{name}: seed {s} meets the margin too"


# --------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", STAGE_IDS)
def test_stage_float32_restatement_passes(name):
    c = cm.STAGE[name]
    err = cm.compare_stage(cm.run_stage_ref(c, F32), cm.run_stage_ref(c, F64), name,
                           need=("y", "amax", "dx", "dw", "db", "dnw") + (("dgamma", "dbeta") if c.ipc else ()))
    print(name, {k: f"{e:.3g}" for k, (e, _) in err.items()})
    assert all(e <= 0.1 * b for k, (e, b) in err.items() if k != "amax")  # an order of magnitude inside the caps


@pytest.mark.parametrize("name", UP_IDS)
def test_up_float32_restatement_passes(name):
    c = cm.UP[name]
    err = cm.compare_stage(cm.run_up_ref(c, F32), cm.run_up_ref(c, F64), name,
                           need=("y", "dx", "dw", "db") + (() if c.last else ("dnw",)))
    print(name, {k: f"{e:.3g}" for k, (e, _) in err.items()})
    assert all(e <= 0.1 * b for e, b in err.values())


@pytest.mark.parametrize("name", KERNEL_IDS)
def test_kernel_float32_restatement_passes(name):
    """rho32, the float32 torch restatement's worst |err| / contraction(|a|, |b|): the f32 arms get 8 x it. It is a
    few float32 roundings (2^-24 = 6e-8 each), far below the split-bf16 arms' 4e-5."""
    c = cm.KERNEL[name]
    kr = cm.run_kernel_ref(c)
    print(f"{name}: rho32 {kr['rho32']:.3g}")
    assert 0 < kr["rho32"] < 1e-6 and cm.F32_SLACK * kr["rho32"] < cm.C_SPLIT
    assert cm.compare_kernel(kr["r32"], kr, c.op, cm.F32_SLACK * kr["rho32"], name) == pytest.approx(kr["rho32"])
    wrong = kr["ref"] + 2 * cm.kernel_bound(kr, c.op, cm.C_SPLIT)  # and an error of twice the widest bound fails
    with pytest.raises(AssertionError):
        cm.compare_kernel(wrong, kr, c.op, cm.C_SPLIT, name)


# --------------------------------------------------------------------------------------------------- the mutants
def _stage_applies(c, mut):
    """whether the mutation can change this case's outputs"""
    return {"pad": c.k % 2 == 0 or c.W > c.k // 2,  # odd: some output column's right-most tap reads column W - 1
            "route": True,
            "dw_rows": c.co % 16 != 0,
            "odd_edge": c.H % 2 == 1 or c.W % 2 == 1}[mut]


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def test_mutations_apply_where_expected():
    off = {m: sorted(c.name for c in cm.STAGE_CASES if not _stage_applies(c, m)) for m in ("pad", "route", "odd_edge")}
    assert off["pad"] == ["hw2_nb3", "hw2_nb32"] and off["route"] == []
    assert sorted(set(STAGE_IDS) - set(off["odd_edge"])) == ["film_hw7", "h21_w16", "hw21", "hw21_c4"]
    partial = sorted(c.name for c in cm.STAGE_CASES if _stage_applies(c, "dw_rows"))
    assert partial == ["co24", "co40", "film_co24", "film_hw7"]
    assert sorted(c.name for c in cm.UP_CASES if c.co % 16) == ["up_3x5_k3", "up_last"]


@pytest.mark.parametrize("mut", ["pad", "route", "dw_rows", "odd_edge"])
@pytest.mark.parametrize("name", STAGE_IDS)
def test_stage_comparison_fails_on_wrong_reference(name, mut):
    c = cm.STAGE[name]
    ref, wrong = cm.run_stage_ref(c, F64), cm.run_stage_ref(c, F64, mut)
    if not _stage_applies(c, mut):  # nothing for the mutation to change here: it must then BE the reference
        assert _same(wrong, ref)
        return
    with pytest.raises(AssertionError):
        cm.compare_stage(wrong, ref, f"{name} {mut}")
    err = cm.stage_errors(wrong, ref)
    if mut in ("route", "dw_rows", "odd_edge"):  # backward-only mutations: the forward still agrees exactly
        assert err["y"][0] < 1e-12 and err["amax"][0] == 0
    if mut != "dw_rows":  # and what the product returns without dx (dw, db, dnw) shows it as well
        assert any(not err[k][0] <= err[k][1] for k in ("y", "dw", "db", "dnw")), err


@pytest.mark.parametrize("mut", ["pad", "ups", "dw_rows"])
@pytest.mark.parametrize("name", UP_IDS)
def test_up_comparison_fails_on_wrong_reference(name, mut):
    c = cm.UP[name]
    ref, wrong = cm.run_up_ref(c, F64), cm.run_up_ref(c, F64, mut)
    if mut == "dw_rows" and c.co % 16 == 0:
        assert _same(wrong, ref)
        return
    with pytest.raises(AssertionError):
        cm.compare_stage(wrong, ref, f"{name} {mut}")


# --------------------------------------------------------------------------------------------------- the plans
def test_plans_agree_with_the_library_at_every_case():
    nat = _native()
    for c in cm.STAGE_CASES:
        cm.check_plans(nat, c.nb, c.H, c.W, c.cx, c.co, c.k)
        cm.check_plans(nat, c.nb, c.H, c.W, c.ci, c.co, c.k)
    for c in cm.UP_CASES:
        cm.check_plans(nat, c.nb, c.H, c.W, c.ci, c.co, c.k, 1)
        cm.check_plans(nat, c.nb, 2 * c.H, 2 * c.W, c.co, c.ci, c.k)
    for c in cm.KERNEL_CASES:
        cm.check_plans(nat, c.nb, c.H, c.W, c.ci, c.co, c.k, c.ups)


def test_plans_agree_with_the_library_over_a_sweep():
    nat = _native()
    sizes = (1, 2, 4, 7, 8, 16, 18, 21, 32, 64, 128, 256)
    channels = ((3, 4, 8, 12, 16, 24, 32, 48, 64, 96), (3, 16, 24, 32, 40, 48, 64, 96))
    for Ci, Co, k in itertools.product(*channels, (3, 4, 5)):
        for H, W in itertools.product(sizes, sizes):
            cm.check_plans(nat, 3 if H * W < 1024 else 1, H, W, Ci, Co, k)
    for Nb in (1, 2, 40, 300, 1024):  # the slab count's two caps: the row blocks and 256 / gx
        for H, W, Ci, Co in ((64, 64, 4, 32), (32, 32, 32, 48), (16, 16, 48, 64), (8, 8, 64, 64), (2, 2, 64, 64)):
            cm.check_plans(nat, Nb, H, W, Ci, Co, 5)


def test_every_reachable_rung_of_the_direct_kernels_is_named_by_a_case():
    """csrc/conv.hip instantiates conv_wgrad_direct / conv_wgrad3_direct<TM, NBW, WS, PL> only at the rungs its four
    plans can reach (WdF32Host::rung, WdBf16x3Host::rung: 23 + 16). The restated plans, enumerated over a grid of
    shapes, reach exactly those, and every one of them is the arm of some case, so the float64 tests launch it."""
    reached = {name: set() for name in ("direct", "direct3", "pool", "pool3")}
    sizes = ((1, 3, 64), (2, 4, 6, 8, 12, 16, 32, 64, 128), [2 ** i for i in range(1, 9)], range(4, 129, 4),
             range(4, 65, 4), (1, 2, 3, 4, 5, 7))
    for Nb, H, W, Ci, Co, k in itertools.product(*sizes):
        plans = dict(direct=cm.direct_plan(Nb, H, W, Ci, Co, k, k), direct3=cm.direct3_plan(Nb, H, W, Ci, Co, k, k),
                     pool=cm.pool_plan(Nb, H, W, Ci, Co, k, k), pool3=cm.pool3_plan(Nb, H, W, Ci, Co, k, k))
        for name, pl in plans.items():
            if pl:
                reached[name].add((pl["tm"], pl["nbw"], pl["ws"]))
    tms = (1, 2, 3, 4)
    want = dict(direct={(tm, nbw, False) for tm in tms for nbw in (2, 4, 7)} | {(tm, 10, False) for tm in (1, 2, 3)}
                | {(tm, 7, True) for tm in tms},
                direct3={(tm, nbw, False) for tm in (1, 2, 3) for nbw in (2, 4, 5, 7)} | {(4, 2, False), (4, 4, False)},
                pool={(tm, 7, True) for tm in tms},
                pool3={(1, 7, True), (2, 7, True)})
    assert reached == want
    assert sum(len(s) for s in want.values()) == 23 + 16
    labels = {c.wgrad.split(" ")[0] for c in cm.STAGE_CASES + cm.UP_CASES}
    labels |= {a.split(" ")[0] for c in cm.KERNEL_CASES if c.op == "wgrad" for a in (c.arm, c.fast) if a}
    for name, rungs in want.items():
        kernel = "conv_wgrad3_direct" if name.endswith("3") else "conv_wgrad_direct"
        for tm, nbw, ws in sorted(rungs):
            arm = f"{kernel}<{tm},{nbw}{',WS' if ws else ''}{',PL' if name.startswith('pool') else ''}>"
            assert arm in labels, f"no case reaches {arm}"


def test_wave_split_plan_reserves_its_reduction_area():
    """A wave-split plan sums its 8 waves' 16 x 16 tiles through 8 KiB of LDS after the last row block: its request
    covers that where the staged block is smaller (a 4 x 4 image of 4 channels stages 2176 bytes)."""
    pl = cm.direct_plan(2, 4, 4, 4, 16, 3, 3)
    assert pl["ws"] and pl["lds"] == cm.WS_REDUCE_BYTES
    assert cm.direct_plan(2, 16, 16, 8, 16, 3, 3)["lds"] > cm.WS_REDUCE_BYTES


def test_pool_rms_refuses_more_than_128_channels_before_any_launch():
    """vpt_for covers 16 lanes x 8 channels: C = 132 is refused by the host (no pointer is read, nothing launched)"""
    nat = _native()
    with pytest.raises(nat.NativeError):
        nat.call("sd_pool_rms_fwd", None, None, None, None, None, None, 2, 4, 4, 132, 1e-4, 0, None)
    with pytest.raises(nat.NativeError):
        nat.call("sd_pool_rms_bwd", None, None, None, None, None, None, None, None, 2, 4, 4, 132, 0, 1, None)
