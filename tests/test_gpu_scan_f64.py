"""RSSM.observe forward and backward (the fused scan csrc/scan.hip where rssm._fused_scan_ok admits the shape, the
per-op HIP kernels elsewhere) against the float64 oracle and its autograd gradient, at the smallest shapes that reach
each kind of instantiation the gate admits (tests/small_models.py; the input condition, the comparison functions and
their discrimination are checked on the CPU by test_small_model_parity_cpu.py).

  case              D    G  SxK    B  T  reaches
  t1_b1_init        256  1  16x32  1  1  T = 1 (no k_carry, one obs/x0p problem), one row, one block; stoch0 / deter0
  t1_b1_reset       256  1  16x32  1  1  the same, the row reset at step 0
  kd64_sk512        1024 4  8x64   5  3  Kd = 64 with SK = 512 (k_logit_rows<64, 1>, k_sbwd_last<64>, k_carry<64>)
  kd64_sk1024_b17   1024 2  16x64  17 3  Kd = 64 with SK = 1024, Dg = 512 below G = 8, a second row tile of one row
  s64               512  2  64x16  3  4  S = 64
  anchor            2048 8  32x16  16 4  the benched shape
  per_op_sk64       512  8  4x16   3  2  outside the gate (Dg = 64, SK = 64): the per-op path at a shape of its own
  per_op_dg96       768  8  4x16   3  2  Dg = 96, no multiple of any kernel's tile: the per-op path

Every case with three rows or more has a row that is never reset and starts from a nonzero initial state, a row reset
at every step, a row reset at step T - 1 only, and rows with random flags.

Compared: the posterior indices (exactly, no row excluded), post_deter and post_logit (1e-4 abs + 1e-3 rel), the
gradient of embed and of every rssm.* parameter (2e-3 of each tensor's max + 1e-7): test_gpu_scan.py's tolerances,
used as caps. The float32 oracle itself sits 2e-7 .. 2e-6 from float64 in the states and 1e-6 of the max in the
gradients; DESIGN.md § 2.1 records the product's figures beside it.
"""
import pytest
import torch

import small_models as sm
from sdreamer import rssm as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def agents():
    made = {}

    def get(name):
        if name not in made:
            made[name] = sm.build_product(sm.SCAN[name])
        return made[name]

    return get


@pytest.mark.parametrize("name", [c.name for c in sm.SCAN_CASES])
def test_observe_matches_float64_oracle(agents, name):
    c = sm.SCAN[name]
    ag = agents(name)
    r = ag.rssm
    assert (r._deter, r._blocks, r._stoch, r._discrete, r._hidden) == (c.D, c.G, c.S, c.K, 256)
    assert R._fused_scan_ok(r, c.B) == c.fused
    got = sm.run_product_scan(ag, c)
    ref = sm.run_oracle_scan(c)
    print(name, sm.scan_summary(sm.scan_errors(got, ref)))
    sm.compare_scan(got, ref, name)


@pytest.mark.parametrize("combo", sm.GRAD_COMBOS, ids=["+".join(g) for g in sm.GRAD_COMBOS])
def test_missing_upstream_gradients(agents, combo):
    """set_materialize_grads(False): an output without a gradient reaches the backward as None. d_deter alone (the
    image-gradient path's use), d_logit alone, d_stoch + d_deter without d_logit — each against the oracle's gradient
    of the same partial loss."""
    c = sm.SCAN["kd64_sk512"]
    got = sm.run_product_scan(agents(c.name), c, combo)
    ref = sm.run_oracle_scan(c, grads=combo)
    print(c.name, combo, sm.scan_summary(sm.scan_errors(got, ref)))
    sm.compare_scan(got, ref, f"{c.name} {combo}")


def _bit_differences(a, b):
    """names of the outputs / gradients whose bits differ, with the count and size of the differences"""
    assert set(a[4]) == set(b[4])
    pairs = list(zip(("post_stoch", "post_deter", "post_logit", "d_embed"), a[:4], b[:4]))
    pairs += [(n, a[4][n], b[4][n]) for n in sorted(a[4])]
    return [(n, int((x != y).sum()), float((x - y).abs().max())) for n, x, y in pairs if not torch.equal(x, y)]


def test_row_tiles_and_repeats_bit_identical_kd64():
    """Kd = 64, B = 17 (two row tiles, the second of one row): the row tile only changes which workgroup computes a
    row, so tiles 16, 8 and 5 give the same bits (as test_gpu_scan.py asserts at the BASELINE shapes), and so do two
    identical calls. k_carry<64> is the one kernel with two sampler elements per thread (rows r and r + 8 of a 16-row
    tile); while each was an inlined copy of the sampler, compiled on its own, rows 8..15 lost this property by one
    ulp in every gradient."""
    c = sm.SCAN["kd64_sk1024_b17"]
    ag = sm.build_product(c)
    assert R._fused_scan_ok(ag.rssm, c.B) and ag.rssm._discrete == 64
    old = R.SCAN_ROW_TILE
    tiles = (0, 0, 8, 5)
    runs = []
    try:
        for rt in tiles:
            R.SCAN_ROW_TILE = rt
            runs.append(sm.run_product_scan(ag, c)["raw"])
    finally:
        R.SCAN_ROW_TILE = old
    bad = {f"run {i} (row tile {rt})": _bit_differences(runs[0], b)
           for i, (rt, b) in enumerate(zip(tiles, runs)) if i and _bit_differences(runs[0], b)}
    assert not bad, bad
