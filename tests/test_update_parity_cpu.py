"""CPU checks of tests/update_models.py, the case module behind tests/test_gpu_update_f64.py:

  * the arm functions restate the dispatch (FlatArena's chunk table is compared with the class itself) and the case
    tables reach every reachable arm;
  * every input condition the GPU comparison relies on holds (column stds, the AGC ratio away from 1 and on both sides
    of it, the pmin arm, exactly representable action edges, rows that reach the stated magnitudes, every byte value),
    and no output of a reference is missing from the restatement: no element is left out of a comparison;
  * the float32 restatement passes every comparison at every case using at most 1/8 of the tolerance (a third where
    the tolerance is the cap itself);
  * a planted fault fails the comparison at every case where it can change the output, and reproduces the float32
    restatement bit for bit where it cannot. One exception, by name (update_models.FAULT_VALID_BELOW): InfoNCE without
    the row maximum is a correct float32 evaluation until exp overflows (88.73), so it must fail at magnitude 100
    and may pass below.
"""
import numpy as np
import pytest
import torch

import update_models as um

F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------ arms
def test_arena_layout_matches_flat_arena():
    from sdreamer.optim import CHUNK, FlatArena
    assert um.CHUNK == CHUNK
    sizes = (1, 3, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)
    ar = FlatArena([torch.nn.Parameter(torch.zeros(n)) for n in sizes], "cpu")
    offs, total, beg, end, tens, t0 = um.arena_layout(sizes)
    assert (ar.offsets, ar.total) == (offs, total)
    assert ar.chunk_beg.tolist() == beg and ar.chunk_end.tolist() == end
    assert ar.chunk_tensor.tolist() == tens and ar.tensor_chunk0.tolist() == t0


def test_barlow_table_reaches_every_arm():
    cases = um.BARLOW_CASES
    for mode in ("fn", "w1"):
        small = [c for c in cases if c.mode == mode and c.Nr < 512]
        assert {(c.Nr, c.E) for c in small} == {(n, e) for n in um.BARLOW_NR for e in um.BARLOW_E}
    # the 64-column block: fewer than 64 columns, exactly 64, a second block of one column, a fifth of one
    assert [um.col_blocks(e) for e in um.BARLOW_E] == [(1, 1), (1, 5), (1, 64), (2, 1), (5, 1)]
    # the CS_NP row partials: fewer rows than partials, one row each, one and two rows, two and three
    assert [um.row_partials(n) for n in um.BARLOW_NR] == [(1, 14), (1, 0), (2, 15), (3, 15)]
    # barlow_partial's grid stride: 257 is the first E that takes a second one
    assert um.barlow_partial_strides(256) == 1 and um.barlow_partial_strides(257) == 2
    assert max(um.barlow_partial_strides(c.E) for c in cases) == 16  # (512, 1024)
    assert {um.rowstats_blocks(e)[1] for e in um.BARLOW_E} == {0, 3}  # idle waves: the j >= E return
    sh = [c for c in cases if c.mode == "sh"]
    assert all(sum(c.shards()) == c.Nr and c.world == 2 for c in sh)
    assert {(c.Nr, c.E) for c in sh if not c.split and c.Nr < 512} == {(n, e) for n in (2, 16) for e in um.BARLOW_E}
    assert [c.shards() for c in sh if c.split] == [(5, 12)]
    assert {c.mode for c in cases if (c.Nr, c.E) == (512, 1024)} == {"fn", "w1", "sh"}
    assert um.BARLOW_G != 1.0


def test_other_tables_reach_every_arm():
    # InfoNCE
    assert {(c.n, c.ncol, c.off) for c in um.NCE_CASES} == set(um.NCE_SHAPES)
    assert {um.nce_row_strides(c.ncol) for c in um.NCE_CASES} == {1, 2, 3}
    assert any(c.ncol % 256 for c in um.NCE_CASES) and any(c.ncol == 256 for c in um.NCE_CASES)
    assert {um.mean_strides(c.n) for c in um.NCE_CASES} == {1, 2}
    assert any(c.off > 0 and c.off + c.n == c.ncol for c in um.NCE_CASES)  # the last admissible label
    assert [c.name for c in um.NCE_CASES if c.ld_extra] == ["n5-c257-o100-ld3"]
    assert all({m for c in um.NCE_CASES if (c.n, c.ncol, c.off) == s and not c.ld_extra for m in (c.mag,)} ==
               set(um.NCE_MAGS) for s in um.NCE_SHAPES)
    with np.errstate(over="ignore"):
        assert 80 < um.EXP_OVERFLOW_F32 < 100 and np.isfinite(np.exp(np.float32(80))) and np.isinf(np.exp(np.float32(100)))
    # metric vector: one element, two, a chunk less one, a whole chunk, one more, three chunks and five
    assert [um.stat_chunks(n) for n in um.STAT_NS] == [(1, 1), (1, 2), (1, 4095), (1, 4096), (2, 1), (4, 5)]
    assert any(c.kind == "offset" for c in um.STAT_CASES)
    # loss terms: the backward's three grids
    assert [len(c.ns) for c in um.LT_CASES] == [1, 3, 8]
    assert {n for c in um.LT_CASES for n in c.ns} == {1, 255, 257, 16383, 16384, 70000}
    assert [um.loss_terms_gx(max(c.ns)) for c in um.LT_CASES] == [1, 64, 64]
    assert max(um.LT_CASES[1].ns) < um.LT_BWD_FULL <= max(um.LT_CASES[2].ns)  # ceil form at its limit, grid stride
    assert 70000 > 64 * 256 * 4  # more than four strides
    k = max(len(c.ns) for c in um.LT_CASES)
    assert any(s != 1.0 for s in um.LT_SCALES[:k]) and any(s < 0 for s in um.LT_SCALES[:k])
    # optimiser
    C = um.CHUNK
    assert set(um.OPT_SIZES) >= {1, 3, 63, 64, 65, C - 1, C, C + 1, 3 * C + 5, 257 * C + 2}
    offs, total, beg, end, tens, t0 = um.arena_layout(um.OPT_SIZES)
    per = [t0[i + 1] - t0[i] for i in range(len(um.OPT_SIZES))]
    assert per == [1, 1, 1, 1, 1, 1, 1, 2, 4, 258]
    assert {um.chunk_sum_strides(n) for n in per} == {1, 2}
    assert total > sum(um.OPT_SIZES)  # padding between tensors exists
    assert any((e - b) % 4 for b, e in zip(beg, end))  # a chunk whose float4 tail runs into the padding
    assert sorted(j for j, s in enumerate(um.OPT_PSCALE) if s == 0.0) == [1, 3]
    assert {c.warmup for c in um.OPT_CASES} == {0, 1000}
    assert {c.variant for c in um.OPT_CASES} == {"plain", "gs", "gate0", "gate1", "zg"}
    assert {n for n, _ in um.POLYAK_CASES} == {1, 255, 257, 100003} and {m for _, m in um.POLYAK_CASES} == {0.02, 1.0}
    # input preparation
    assert um.PREP_NS == (1, 255, 257) and set(um.U8_CP) == {(1, 1), (1, 4), (3, 4), (4, 4), (3, 8)}


def test_slice_table_reaches_every_arm():
    paths = {k[0]: um.slice_key_paths(k) for k in um.SL_KEYS}
    assert paths["vec16"] == {"vector"} and paths["initial"] == {"vector"} and paths["action"] == {"vector"}
    assert paths["b1"] == paths["b12"] == paths["b20"] == {"bytes"}  # row_bytes 1, 12, 20
    assert paths["mis16"] == {"bytes"}  # 16-byte rows at a 4-byte aligned base
    by = {k[0]: k for k in um.SL_KEYS}
    assert {np.dtype(k[1]).itemsize * k[2] for k in um.SL_KEYS} >= {1, 12, 16, 20}
    assert by["initial"][3:5] == (1, 0) and by["action"][3:5] == (um.SL_L, 0)
    assert (um.SL_CAP, um.SL_E, um.SL_L) == (7, 2, 3)
    assert any(um.SL_STARTS[p][0] + 1 + j >= um.SL_CAP for p in um.SL_PICK for j in range(um.SL_L))  # the wrap
    ref = um.ref_slices_gather()
    assert ref["t_idx"].max() == um.SL_CAP - 1 and ref["t_idx"].min() == 0 and set(ref["e_idx"].ravel()) == {0, 1}
    _, cnt = um.ref_slices_scatter(4)
    assert {0, 1, 2, 3} <= set(cnt.ravel())  # untouched rows, rows of one writer, of two and of three
    # the faults change something
    bad = um.ref_slices_gather("action_shift_1")
    assert not np.array_equal(bad["action"], ref["action"])
    assert all(np.array_equal(bad[k], ref[k]) for k in ref if k != "action")
    a, b = um.ref_slices_scatter(4)[0], um.ref_slices_scatter(4, "smallest_b_wins")[0]
    assert ((a != b).any(-1) == (cnt > 1)).all()  # every row of several writers, and only those


# ------------------------------------------------------------------------------------------------ input conditions
def test_barlow_columns_are_wide():
    for c in um.BARLOW_CASES:
        i = um.barlow_inputs(c)
        for k in ("x1", "x2"):
            assert float(i[k].double().std(0).min()) >= um.BARLOW_MIN_STD, (c.name, k)
        if c.mode != "fn":
            assert float(i["s1r"].min()) >= um.BARLOW_MIN_STD


def test_infonce_rows_reach_their_magnitude():
    for c in um.NCE_CASES:
        i = um.nce_inputs(c)
        l = i["logits"]
        if c.mag:
            assert float(l.abs().max()) == c.mag
            if c.ncol > 1:
                assert bool((l.max(1).values == c.mag).all()) and bool((l.min(1).values == -c.mag).all())
            lf = i["x1"].double() @ i["x2g"].double().t()
            assert abs(float(lf.abs().max()) - c.mag) < 1e-3
        assert 0 <= c.off and c.off + c.n <= c.ncol


def test_optimiser_conditions():
    i = um.opt_inputs()
    assert all(not bool(i["p"][j].any()) for j in (1, 3)) and um.OPT_SIZES[1] < 4
    assert all(not bool(i["g"][it][um.OPT_ZERO_GRAD].any()) for it in range(um.OPT_STEPS))
    for c in um.OPT_CASES:
        if c.variant == "zg":  # the reference does not depend on zero_grads
            continue
        r = um.ref_optim(c, scales=False)
        for it in range(um.OPT_STEPS):
            ratio = r[f"@ratio{it}"]
            assert np.abs(ratio - 1).min() >= um.AGC_MARGIN, (c.name, it, ratio)
        r2 = r["@ratio1"]
        assert (r2 > 1).any() and (r2[[j for j in range(len(r2)) if j != um.OPT_ZERO_GRAD]] < 1).any(), r2
        assert (r["@ratio0"][[1, 3]] > 1).all()  # the pmin arm clips: ||p|| = 0 < pmin
        assert r["@ratio0"][um.OPT_ZERO_GRAD] == 0
        if c.warmup:
            assert r["scalars0"][3] < r["scalars1"][3] < r["scalars2"][3]
        assert [r[f"scalars{it}"][0] for it in range(3)] == [1, 2, 3]


def test_prep_inputs():
    assert all(float(np.float32(v)) == v for v in um.ACTION_EDGES)  # the branch |a| > 1 is the same in both types
    assert um.ONE_DN < 1 < um.ONE_UP
    for n in um.PREP_NS:
        i = um.prep_inputs(n)
        if n >= len(um.ACTION_EDGES):
            assert i["symlog"][:len(um.SYMLOG_EDGES)].tolist() == [float(np.float32(v)) for v in um.SYMLOG_EDGES]
            assert i["action"][:len(um.ACTION_EDGES)].tolist() == list(um.ACTION_EDGES)
            assert set(i["last"].tolist()) == set(um.FLAG_BYTES) == set(i["termb"].tolist())
            for w in (1, 7):
                for st in (1, 3):
                    m = i[f"mask{w}s{st}"]
                    assert m.numel() == n * st and set(m[::st].tolist()) == set(um.MASK_BYTES)
        assert i["bytes"].tolist() == list(range(256))
    for c in um.STAT_CASES:
        a = um.stat_inputs(c)["a"].double()
        if c.kind == "offset":
            assert abs(float(a.mean()) - 100) < 0.1 and abs(float(a.std()) - 1) < 0.1


def test_no_output_is_left_out():
    for fam, (cases, fn) in um.FAMILIES.items():
        if fam == "optim":
            continue  # test_float32_restatement_passes_with_room asserts it there
        c = cases[-1]
        ref, got = um.reference(fam, c), fn(c, F32)
        assert set(um.outputs(ref)) == set(um.outputs(got)), fam
        assert all(um.base_name(fam, k) in um.TOL[fam] for k in um.outputs(ref)), fam
    for c in um.BARLOW_CASES:
        assert set(um.outputs(um.reference("barlow", c))) == set(um.BARLOW_OUTPUTS[c.mode])


def test_restated_optimiser_is_the_oracle():
    c = um.OPT["w1000-gate1"]
    for dt in (F32, F64):
        a, b = um.ref_optim(c, dt, scales=False), um.ref_optim(c, dt, restated=True, scales=False)
        assert um.same_bits(a, b)


# ------------------------------------------------------------------------------------------------ the comparison
def _room(fam, worst):
    # an "ulp" tolerance is the issue's own figure, filled by IEEE's half ulp per rounding: no room to ask for
    return {k: 1.0 if um.tol_of(fam, k).kind == "ulp" else 1 / 3 if um.tol_of(fam, k).capped else 0.125 for k in worst}


@pytest.mark.parametrize("fam", [f for f in um.FAMILIES if f != "optim"])
def test_float32_restatement_passes_with_room(fam):
    cases, fn = um.FAMILIES[fam]
    worst = {}
    for case in cases:
        ref, got = um.reference(fam, case), fn(case, F32)
        um.compare(fam, got, ref, f"{fam} {um.case_name(case)}")
        for k, (a, b) in um.ratios(fam, got, ref).items():
            k = um.base_name(fam, k)
            worst[k] = max(worst.get(k, (0, 0)), (a, b, um.case_name(case)))
    print(fam, {k: f"{a:.3g} of the bound, {b:.3g} of the cap ({n})" for k, (a, b, n) in worst.items()})
    room = _room(fam, worst)
    assert all(a <= room[k] and b <= room[k] for k, (a, b, _) in worst.items()), worst


@pytest.mark.parametrize("fam,fault", [(f, x) for f, xs in um.FAULTS.items() if f != "optim" for x in xs])
def test_planted_fault_fails(fam, fault):
    cases, fn = um.FAMILIES[fam]
    caught, same, valid = [], [], []
    for case in cases:
        ref, base, bad = um.reference(fam, case), fn(case, F32), fn(case, F32, fault)
        name = um.case_name(case)
        if um.same_bits(base, bad):
            same.append(name)
        elif fault in um.FAULT_VALID_BELOW and um.FAULT_VALID_BELOW[fault](case):
            valid.append(name)
        else:
            assert not um.passes(fam, bad, ref), f"{fault} changes {fam} {name} and is not caught"
            caught.append(name)
    print(fam, fault, "caught at", len(caught), "cases; cannot change", len(same), same[:12], "; a valid evaluation at",
          len(valid))
    assert caught
    if fault in um.FAULT_VALID_BELOW:
        assert all(not um.FAULT_VALID_BELOW[fault](c) for c in cases if um.case_name(c) in caught)
        assert any(um.case_name(c) in caught for c in cases if not um.FAULT_VALID_BELOW[fault](c))


def test_optimiser_restatement_and_faults():
    """Per case one float64 reference (0.5 GB), the float32 restatement within 1/8 of every tolerance, and every fault:
    failing where it changes a bit, the restatement bit for bit elsewhere. `step_not_advanced` shows at warm-up 1000
    only (without a warm-up the learning rate does not read the step)."""
    worst, caught = {}, {f: [] for f in um.FAULTS["optim"]}
    for c in um.OPT_CASES:
        if c.variant == "zg":  # the same reference as the plain case
            continue
        ref, base = um.ref_optim(c), um.ref_optim(c, F32, scales=False)
        assert set(um.outputs(ref)) == set(um.outputs(base))
        um.compare("optim", base, ref, f"optim {c.name}")
        for k, (a, b) in um.ratios("optim", base, ref).items():
            k = um.base_name("optim", k)
            worst[k] = max(worst.get(k, (0, 0)), (a, b, c.name))
        for fault in um.FAULTS["optim"]:
            bad = um.ref_optim(c, F32, fault, scales=False)
            if um.same_bits(base, bad):
                continue
            assert not um.passes("optim", bad, ref), f"{fault} changes optim {c.name} and is not caught"
            caught[fault].append(c.name)
    print("optim", {k: f"{a:.3g} of the bound, {b:.3g} of the cap ({n})" for k, (a, b, n) in worst.items()}, caught)
    room = _room("optim", worst)
    assert all(a <= room[k] and b <= room[k] for k, (a, b, _) in worst.items()), worst
    assert all(caught.values()), caught
    assert caught["step_not_advanced"] and all(n.startswith("w1000") for n in caught["step_not_advanced"])
    assert set(caught["gate_after_norm"]) == {"w1000-gate0"}  # gate 1 multiplies by one: the same bits
    assert len(caught["agc_no_pmin"]) == len(caught["clip_from_chunk"]) == len(caught["bc1_not_over_lr"]) == 5
