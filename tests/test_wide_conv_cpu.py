"""CPU self-check of the wide conv stage tests (tests/wide_conv_models.py; tests/test_gpu_wide_conv_f64.py runs the same
cases and comparisons on the product), in the manner of test_conv_parity_cpu.py:

1. the tie margin per stage case (smallest float64 window margin >= 32 x the float32 restatement's conv error, float32
   and float64 argmax equal), with the seed re-derived as the first that meets it;
2. the float32 restatement passes every comparison;
3. the comparisons fail on wrong float64 references: conv_models.MUTANTS where they apply, the RMS sum taken over the
   first 128 channels only, the contraction's last K % 32 products dropped, the output columns from 64 floor(N / 64)
   zeroed, a pixel slab skipped. Where a mutant cannot change a case it must EQUAL the reference;
4. the new host-only queries and the refusals (width 513, narrow widths) answer before any pointer is read;
5. a stage width above 512 is refused when the encoder is constructed.
"""
import copy

import numpy as np
import pytest

import conv_models as cm
import wide_conv_models as wm

F32, F64 = cm.F32, cm.F64
STAGE_IDS = [c.name for c in wm.STAGE_CASES]
KERNEL_IDS = [c.name for c in wm.KERNEL_CASES]


def _native():
    try:
        from sdreamer import _native as nat
    except ImportError:
        pytest.skip("libsdhip.so is not built")
    return nat


def test_cases_cover_the_new_paths():
    S, Kc = wm.STAGE_CASES, wm.KERNEL_CASES
    assert all(c.co > wm.WIDE_MIN and c.co <= wm.WIDE_MAX for c in S)
    assert {129, 512} <= {c.co for c in S} and any(c.co % 2 for c in S)  # both ends of the range, an odd width
    assert any(c.co <= 256 for c in S) and any(c.co > 256 for c in S)  # 4 and 8 channels per lane
    assert any(c.raw and c.dx for c in S) and any(c.ipc for c in S) and any(c.nchw for c in S)
    assert any(c.H // 2 * 2 != c.H or c.W // 2 * 2 != c.W or (c.H // 2) % 2 for c in S)
    assert any((c.H // 2) % 2 == 1 and c.nb * c.H * c.W % wm.BM for c in S)  # odd pooled edge, ragged M tile
    for op in ("dgrad", "wgrad"):
        assert all(wm.kernel_mutant_applies(c, "k_tail") for c in Kc if c.name in ("kd_s1", "kw_231_308"))
        assert any(wm.kernel_mutant_applies(c, "n_tail") for c in Kc if c.op == op)
        assert any(c.nb * c.H * c.W > wm.BM for c in Kc if c.op == op)
    assert (25 * 154) % 32 and (25 * 154) % 4  # K = 3850
    assert wm.kernel_mutant_applies(wm.KERNEL["kw_slabs"], "slab")
    for c in S:
        assert wm.stage_arms(c) == (c.fwd, c.wgrad, c.dgrad)
        assert c.fwd.startswith("conv_fwd_kernel<128,64") and cm.fused_fwd_arm(c.nb, c.H, c.W, c.cx, c.co, c.k) is None
        # every older fast arm refuses these shapes
        assert cm.direct3_plan(c.nb, c.H, c.W, c.cx, c.co, c.k, c.k) is None
        assert cm.pool_plan(c.nb, c.H, c.W, c.cx, c.co, c.k, c.k) is None
        assert cm.dgrad_arm(c.H, c.W, c.co, c.cx, c.k).startswith("conv_fwd_kernel")
    for c in Kc:
        assert wm.wide_takes(c.ci, c.co) and cm.kernel_arms(c) == (c.arm, "")  # conv_models knows no fast arm here


# --------------------------------------------------------------------------------------------------- the tie margin
@pytest.mark.parametrize("name", STAGE_IDS)
def test_stage_inputs_have_no_near_ties(name):
    c = wm.STAGE[name]
    r32, r64 = cm.run_stage_ref(c, F32), cm.run_stage_ref(c, F64)
    err = wm.conv_err(c)
    print(f"{name}: smallest window margin {r64['margin']:.3g}, float32 conv error {err:.3g}")
    assert r64["margin"] >= cm.MARGIN_FACTOR * err, f"{name}: margin {r64['margin']:.3g} < 32 x {err:.3g}"
    assert np.array_equal(r32["amax"], r64["amax"])
    assert c.seed < cm.MAX_SEEDS
    for s in range(c.seed):  # the seed is the first that meets the rule, chosen from the reference alone
        e = cm.with_seed(c, s)
        r = cm.run_stage_ref(e, F64)
        same = np.array_equal(cm.run_stage_ref(e, F32)["amax"], r["amax"])
        assert r["margin"] < cm.MARGIN_FACTOR * wm.conv_err(e) or not same, f"{name}: seed {s} meets the rule too"


# --------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", STAGE_IDS)
def test_stage_float32_restatement_passes(name):
    c = wm.STAGE[name]
    err = cm.compare_stage(cm.run_stage_ref(c, F32), cm.run_stage_ref(c, F64), name,
                           need=("y", "amax", "dx", "dw", "db", "dnw") + (("dgamma", "dbeta") if c.ipc else ()))
    print(name, {k: f"{e:.3g}/{b:.3g}" for k, (e, b) in err.items()})


@pytest.mark.parametrize("name", KERNEL_IDS)
def test_kernel_float32_restatement_passes(name):
    c = wm.KERNEL[name]
    kr = cm.run_kernel_ref(c)
    print(f"{name}: rho32 {kr['rho32']:.3g}")
    assert 0 < kr["rho32"] < 1e-6 and cm.F32_SLACK * kr["rho32"] < cm.C_SPLIT
    assert cm.compare_kernel(kr["r32"], kr, c.op, cm.F32_SLACK * kr["rho32"], name) == pytest.approx(kr["rho32"])
    wrong = kr["ref"] + 2 * cm.kernel_bound(kr, c.op, cm.C_SPLIT)
    with pytest.raises(AssertionError):
        cm.compare_kernel(wrong, kr, c.op, cm.C_SPLIT, name)


# --------------------------------------------------------------------------------------------------- the mutants
def _stage_applies(c, mut):
    return {"pad": c.k % 2 == 0 or c.W > c.k // 2, "route": True, "dw_rows": c.co % 16 != 0,
            "odd_edge": c.H % 2 == 1 or c.W % 2 == 1}[mut]


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def test_mutations_apply_where_expected():
    assert [c.name for c in wm.STAGE_CASES if not _stage_applies(c, "pad")] == ["w_308_308"]
    assert [c.name for c in wm.STAGE_CASES if _stage_applies(c, "odd_edge")] == []  # H and W even: the pooled edge
    assert sorted(c.name for c in wm.STAGE_CASES if not _stage_applies(c, "dw_rows")) == ["w_96_512"]


@pytest.mark.parametrize("mut", ["pad", "route", "dw_rows", "odd_edge"])
@pytest.mark.parametrize("name", STAGE_IDS)
def test_stage_comparison_fails_on_wrong_reference(name, mut):
    assert mut in cm.MUTANTS
    c = wm.STAGE[name]
    ref, wrong = cm.run_stage_ref(c, F64), cm.run_stage_ref(c, F64, mut)
    if not _stage_applies(c, mut):
        assert _same(wrong, ref)
        return
    with pytest.raises(AssertionError):
        cm.compare_stage(wrong, ref, f"{name} {mut}")


@pytest.mark.parametrize("name", STAGE_IDS)
def test_stage_comparison_fails_on_a_128_channel_rms_sum(name):
    c = wm.STAGE[name]
    ref, wrong = cm.run_stage_ref(c, F64), wm.run_stage_rms128(c)
    with pytest.raises(AssertionError):
        cm.compare_stage(wrong, ref, f"{name} rms128")
    err = cm.stage_errors(wrong, ref)
    assert not err["y"][0] <= err["y"][1] and not err["dnw"][0] <= err["dnw"][1] and err["amax"][0] == 0


@pytest.mark.parametrize("mut", wm.KERNEL_MUTANTS)
@pytest.mark.parametrize("name", KERNEL_IDS)
def test_kernel_comparison_fails_on_wrong_reference(name, mut):
    c = wm.KERNEL[name]
    kr, wrong = cm.run_kernel_ref(c), wm.run_kernel_mutant(c, mut)
    if not wm.kernel_mutant_applies(c, mut):
        assert np.array_equal(wrong, kr["ref"])
        return
    with pytest.raises(AssertionError):
        cm.compare_kernel(wrong, kr, c.op, cm.C_SPLIT, f"{name} {mut}")


# --------------------------------------------------------------------------------------------------- the host queries
def test_wide_queries_answer_without_a_pointer():
    nat = _native()
    q = nat.fns
    for c in wm.STAGE_CASES + wm.KERNEL_CASES:
        cx = getattr(c, "cx", c.ci)
        pad = c.k - 1 - (c.k - 1) // 2
        assert q["sd_conv2d_dgrad_wide3_ok"](c.nb, c.H, c.W, c.co, cx, c.k, c.k, pad) == 1, c.name
        takes = wm.wgrad_takes(cx, c.co)  # a first stage's few input channels stay on the f32 tiles
        want = wm.auto_slabs(c.nb, c.H, c.W, cx, c.co, c.k) if takes else 0
        assert q["sd_conv2d_wgrad_wide3_slabs"](c.nb, c.H, c.W, cx, c.co, c.k, c.k, 0) == want, c.name
        ktiles = -(-c.nb * c.H * c.W // wm.BK)
        for req in (1, 3, 1000):
            want = min(req, ktiles) if takes else 0
            assert q["sd_conv2d_wgrad_wide3_slabs"](c.nb, c.H, c.W, cx, c.co, c.k, c.k, req) == want
    assert wm.auto_slabs(1024, 32, 32, 154, 231, 5) == 9 and wm.auto_slabs(1024, 8, 8, 308, 308, 5) == 3
    assert q["sd_conv2d_wgrad_wide3_slabs"](1024, 32, 32, 154, 231, 5, 5, 0) == 9
    assert [ci for ci in (4, 32, 63, 64, 96) if q["sd_conv2d_wgrad_wide3_slabs"](2, 8, 8, ci, 154, 5, 5, 0)] == [64, 96]
    assert nat._define(nat.HEADER, "SD_WIDE3_WGRAD_MIN_CI") == wm.WGRAD_MIN_CI
    assert sorted(c.name for c in wm.STAGE_CASES + wm.KERNEL_CASES
                  if not wm.wgrad_takes(getattr(c, "cx", c.ci), c.co)) == ["kd_s1", "kw_s1", "w_s1_dx"]
    # both channel counts <= 128: not the wide arms' (every existing route stays), whatever else holds
    for ci, co in ((128, 128), (96, 128), (128, 64), (3, 32), (64, 64)):
        assert not wm.wide_takes(ci, co)
        assert q["sd_conv2d_dgrad_wide3_ok"](2, 8, 8, co, ci, 5, 5, 2) == 0
        assert q["sd_conv2d_wgrad_wide3_slabs"](2, 8, 8, ci, co, 5, 5, 0) == 0
        assert q["sd_conv2d_wgrad_wide3_slabs"](2, 8, 8, ci, co, 5, 5, 3) == 0
        with pytest.raises(nat.NativeError):
            nat.call("sd_conv2d_dgrad_wide3", None, None, None, 2, 8, 8, co, ci, 5, 5, 2, None)
        with pytest.raises(nat.NativeError):
            nat.call("sd_conv2d_wgrad_wide3", None, None, None, None, 0, 0, 2, 8, 8, ci, co, 5, 5, 2, None, None)
    assert q["sd_conv2d_dgrad_wide3_ok"](2, 8, 8, 129, 4, 5, 5, 2) == 1 and q["sd_conv2d_dgrad_wide3_ok"](
        2, 8, 8, 4, 129, 5, 5, 2) == 1
    assert q["sd_conv2d_dgrad_wide3_ok"](1 << 20, 64, 64, 154, 4, 5, 5, 2) == 0  # the pixel count leaves the int range


def test_wide_row_entries_refuse_other_widths_before_any_launch():
    """129 .. 512 channels are the wide entries'; every other width is refused by the host with null pointers (no
    pointer is read, nothing launched), 513 included. The narrow entries keep refusing above 128."""
    nat = _native()
    from sdreamer import kernels as K
    assert (K.WIDE_ROWS_MIN, K.WIDE_ROWS_MAX) == (wm.WIDE_MIN, wm.WIDE_MAX)
    for C in (513, 128, 64, 0, 1024):
        with pytest.raises(nat.NativeError):
            nat.call("sd_pool_rms_wide_fwd", None, None, None, None, None, None, 2, 4, 4, C, 1e-4, 0, None)
        with pytest.raises(nat.NativeError):
            nat.call("sd_pool_rms_wide_fwd_film", None, None, None, None, 1, None, None, None, None, 2, 4, 4, C, 1e-4,
                     0, None)
        with pytest.raises(nat.NativeError):
            nat.call("sd_pool_rms_wide_bwd", None, None, None, None, None, None, None, None, 2, 4, 4, C, 0, 1, None)
        with pytest.raises(nat.NativeError):
            nat.call("sd_pool_rms_wide_bwd_film", None, None, None, None, None, 1, None, None, None, None, None, None,
                     None, None, 2, 4, 4, C, 0, 1, None)
    with pytest.raises(nat.NativeError):
        nat.call("sd_pool_rms_fwd", None, None, None, None, None, None, 2, 4, 4, 231, 1e-4, 0, None)
    q = nat.fns
    assert q["sd_pool_rms_wide_bwd_blocks"](2, 8, 8) == 8 and q["sd_pool_rms_wide_bwd_blocks"](1024, 64, 64) == 2048
    assert q["sd_pool_rms_wide_bwd_blocks"](1, 1, 8) == 1
    assert q["sd_film_grad_wide_floats"](4, 2, 4, 4, 132) == 2 * 2 * 2 * 132
    assert q["sd_film_grad_wide_floats"](64, 32, 64, 64, 154) == 2 * 64 * 2 * 154


# --------------------------------------------------------------------------------------------------- the encoder
def _spaces():
    class Sp:
        def __init__(self, s):
            self.shape = tuple(s)

    class Spaces:
        spaces = {"image": Sp((64, 64, 3))}
    return Spaces(), Sp((6,))


def test_a_stage_width_above_512_is_refused_at_construction():
    _native()
    from sdreamer import networks
    from sdreamer.config import load_config
    from sdreamer.dreamer import Dreamer
    cfg = load_config("dmc/cnn", ["model.depth=129"])  # stages 258 / 387 / 516 / 516
    with pytest.raises(NotImplementedError, match="512"):
        networks.ConvEncoder(cfg.model.encoder.cnn, (64, 64, 3))
    obs, act = _spaces()
    with pytest.raises(NotImplementedError, match="512"):
        Dreamer(copy.deepcopy(cfg.model), obs, act)
    for depth, widths in ((128, (256, 384, 512, 512)), (77, (154, 231, 308, 308))):
        cfg = load_config("dmc/cnn", [f"model.depth={depth}"])
        enc = networks.ConvEncoder(cfg.model.encoder.cnn, (64, 64, 3))
        assert enc.depths == widths and enc.out_dim == widths[-1] * 16


def test_the_wider_cnn_config_is_the_reference_width():
    from sdreamer.config import load_config
    cfg = load_config("dmc/wider_cnn")
    base = load_config("dmc/cnn")
    assert int(cfg.model.depth) == 77 and int(cfg.model.encoder.cnn.depth) == 77
    assert cfg.model.use_multimodal_encoder is False
    assert [77 * int(m) for m in cfg.model.encoder.cnn.mults] == [154, 231, 308, 308]
    assert float(cfg.model.lr) == float(base.model.lr) and cfg.env.task == base.env.task
