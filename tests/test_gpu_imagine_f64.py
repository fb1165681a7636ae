"""Dreamer._imagine_tm (the fused imagination csrc/img.hip where Dreamer._fused_imag_ok admits the shape, the per-op
HIP kernels elsewhere) against Oracle.imagine in float64, at shapes where csrc/img.hip's iplan() makes each of its
kernel sets the default path — not only behind the environment switches of test_gpu_imagine.py at the BASELINE sizes
(tests/small_models.py; checked on the CPU by test_small_model_parity_cpu.py).

  case            D    G  SxK    actor                 img  N    H1  default plan, and what else it reaches
  dg64            512  8  4x16   continuous A6, 3 lay. 2    65   3   k_hid<true> + k_lin6; Dg = 64; a row tile of one row
  sk64_a16        128  2  2x32   continuous A16, 1 l.  4    1    4   the same; smallest SK, Kd = 32, 2A = 32 logits, N = 1
  s68_onehot16    256  4  68x16  one-hot A16, 3 lay.   2    70   3   S > 64: no pre-split images, k_hid<false> + fp32 k_lin
  dg256_onehot1   1024 4  32x32  one-hot A1, 4 layers  1    130  3   k_hid_areg + k_lin6; three row tiles, the last of two rows
  areg_h2         2048 8  32x16  continuous A1, 3 lay. 2    64   2   k_hid_areg + k_lin6_areg at their shortest horizon
  per_op_dg96     768  8  4x16   continuous A6         2    65   3   Dg = 96: refused by the gate, the per-op path
  per_op_dg32     256  8  4x16   continuous A6         2    65   3   Dg = 32: the same

Compared at every step: the imagined stoch indices and one-hot actions (exactly, no row excluded), deter and the
actions (1e-3 rel + 2e-4 abs, test_gpu_imagine.py's tolerance used as a cap). The rows' noise counters start at
global row 3 (row_offset).
"""
import pytest

import small_models as sm
from sdreamer import _native as nat

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c.name for c in sm.IMAG_CASES])
def test_imagine_matches_float64_oracle(name):
    c = sm.IMAG[name]
    ag = sm.build_product(c)
    r = ag.rssm
    assert (r._deter, r._blocks, r._stoch, r._discrete, r._img_layers) == (c.D, c.G, c.S, c.K, c.img_layers)
    assert (ag.act_dim, ag.act_discrete, ag.actor.mlp.n) == (c.A, c.discrete, c.actor_layers)
    assert ag._fused_imag_ok() == c.fused
    assert sm.imag_plan(c) == c.plan  # which kernels csrc/img.hip's iplan() launches by default at this shape
    got = sm.run_product_imag(ag, c)
    ref = sm.run_oracle_imag(c)
    print(name, sm.imag_errors(got, ref, c.discrete))
    sm.compare_imag(got, ref, c.discrete, name)


@pytest.mark.parametrize("name", ["per_op_dg32", "per_op_dg96"])
def test_gates_refuse_blocks_no_multiple_of_64(name):
    """k_hid / k_hid_areg take 64-column tiles and read the block as n0 / Dg: Dg = 32 leaves no tile per block (a
    division by zero on the device), Dg = 96 makes a tile straddle two blocks. Both sides of the gate refuse them —
    the library when asked for the workspace, before any launch."""
    c = sm.IMAG[name]
    assert c.Dg % 64
    ag = sm.build_product(c)
    assert not ag._fused_imag_ok()
    n = sm.imagine_work_status(c.D, c.G, c.S, c.K, c.A, c.discrete, c.actor_layers, c.img_layers, c.N, c.H1)
    assert n == nat.SD_ESHAPE
    with pytest.raises(nat.NativeError):  # and the product's own descriptor is refused the same way
        ag._imagine_prepare(c.N, c.H1, 0, 0, "cuda")
