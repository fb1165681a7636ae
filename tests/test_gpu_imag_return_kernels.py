"""The three kernels of the imagined return's backward (sd_lambda_return_bwd, sd_twohot_mode_bwd,
sd_bnormal_sample_bwd), each against float64 torch autograd of the oracle's formula, at the smallest shapes at which
each can still go wrong."""
import pytest
import torch

import imag_return_ref as irr
import small_models as sm
from oracle import noise as nz
from oracle import ref_cpu as R
from test_gpu_ops import close

pytestmark = pytest.mark.gpu
DEV = "cuda"
DISC = 1 - 1 / 333
MIN_STD, MAX_STD = 0.1, 1.0
BN_SEED, BN_STEP, BN_ROW_OFFSET = 0, 2, 3  # BN_SEED: see test_bnormal_sample_bwd


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ lambda return
@pytest.mark.parametrize("lamb", [0.0, 0.95, 1.0])
@pytest.mark.parametrize("N,T", [(1, 2), (3, 5), (65, 16)])
@pytest.mark.parametrize("dense", [False, True], ids=["col0", "dense"])
def test_lambda_return_bwd(N, T, lamb, dense):
    from sdreamer import kernels as K
    g = _g(100 * N + T)
    rew, val, cl = torch.randn(T, N, generator=g), torch.randn(T, N, generator=g), 2 * torch.randn(T, N, generator=g)
    d_ret = torch.randn(N, T - 1, generator=g)
    if not dense:
        d_ret[:, 1:] = 0
    r64, v64, c64 = (x.t().double().requires_grad_(True) for x in (rew, val, cl))  # (N, T)
    cont = torch.sigmoid(c64)
    ret = irr.lambda_return_diff(1 - cont, r64, v64, v64, DISC, lamb)
    want = torch.autograd.grad((ret * d_ret.double()).sum(), [r64, v64, c64])
    tm = [x.to(DEV) for x in (rew, val, cl)]  # time-major, as the imagined heads write them
    fwd = K.lambda_return(tm[0].t(), tm[1], DISC, lamb, cont_logit=tm[2].t(), boot_row_stride=1, boot_t_stride=N)
    close(fwd, ret, 1e-5, "forward (the recurrence the reference restates)")
    got_tm = K.lambda_return_bwd(d_ret.to(DEV), tm[0].t(), tm[1].t(), tm[2].t(), DISC, lamb, time_major=True)
    rm = [x.t().contiguous() for x in tm]
    got_rm = K.lambda_return_bwd(d_ret.to(DEV), rm[0], rm[1], rm[2], DISC, lamb)
    torch.cuda.synchronize()
    for name, a, b, w in zip(("d_reward", "d_value", "d_cont_logit"), got_tm, got_rm, want):
        assert a.shape == (T, N) and b.shape == (N, T)
        assert torch.equal(a.t(), b), f"{name}: the strided and the row-major reads differ"
        assert not bool(b[:, 0].any()), f"{name}: column 0 takes no gradient"
        close(b, w, 1e-5, name)


# ------------------------------------------------------------------------------------------------ two-hot mode
@pytest.mark.parametrize("rows", [1, 65])
@pytest.mark.parametrize("kind", ["peaked", "flat", "outermost"])
def test_twohot_mode_bwd(rows, kind):
    from sdreamer import kernels as K
    NB = 255
    g = _g(rows + len(kind))
    bins = R.twohot_bins(NB).float()
    logits = {"peaked": 8.0, "flat": 0.01, "outermost": 1.0}[kind] * torch.randn(rows, NB, generator=g)
    if kind == "outermost":  # one row with its mass on the two outermost bins (the +- 4.8e8 pair cancels in the mode)
        logits[0] = -30.0
        logits[0, 0], logits[0, NB - 1] = 3.0, 2.5
    d_out = torch.randn(rows, generator=g)
    l64 = logits.double().requires_grad_(True)
    with sm.oracle_dtype(torch.float64):
        mode = R.twohot_mode(l64, bins.double()).squeeze(-1)
    (want,) = torch.autograd.grad((mode * d_out.double()).sum(), l64)
    lg, bn = logits.to(DEV), bins.to(DEV)
    got = K.twohot_mode_bwd(lg, bn, d_out.to(DEV))
    torch.cuda.synchronize()
    assert got.shape == (rows, NB)
    close(got, want, 1e-5, f"d_logits ({kind})")


def test_twohot_mode_bwd_refuses_even_and_wide_rows():
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    x = torch.zeros(2, 254, device=DEV)
    with pytest.raises(nat.NativeError):
        K.twohot_mode_bwd(x, torch.zeros(254, device=DEV), torch.zeros(2, device=DEV))
    x = torch.zeros(2, 257, device=DEV)
    with pytest.raises(nat.NativeError):
        K.twohot_mode_bwd(x, torch.zeros(257, device=DEV), torch.zeros(2, device=DEV))


# ------------------------------------------------------------------------------------------------ bounded normal
def _bn_inputs(rows, A):
    g = _g(31 * rows + A)
    x = 1.5 * torch.randn(rows, 2 * A, generator=g)
    d_an = torch.randn(rows, A, generator=g)
    eps = torch.from_numpy(nz.normal_block(BN_SEED, nz.STREAM_ACT, BN_STEP, rows, BN_ROW_OFFSET, A))
    return x, d_an, eps


def _bn_action(x, eps):
    """float64: (sampled action, normalised action) of the oracle's formulas"""
    with sm.oracle_dtype(torch.float64):
        loc, sc = R.bounded_normal_params(x, MIN_STD, MAX_STD)
    a = loc + eps.double() * sc
    return a, a / torch.clip(torch.abs(a), min=1.0).detach()


@pytest.mark.parametrize("rows", [1, 65])
@pytest.mark.parametrize("A", [1, 6, 16])
def test_bnormal_sample_bwd(rows, A):
    """BN_SEED was chosen on the CPU (the first of 0, 1, 2, ... at which every (rows, A) here draws at least one
    |action| > 1), so the clip's constant divisor is exercised in every case; asserted below."""
    from sdreamer import kernels as K
    x, d_an, eps = _bn_inputs(rows, A)
    x64 = x.double().requires_grad_(True)
    a64, an64 = _bn_action(x64, eps)
    assert bool((a64.abs() > 1.0 + 1e-3).any()) and (rows * A == 1 or bool((a64.abs() < 1.0 - 1e-3).any()))
    (want,) = torch.autograd.grad((an64 * d_an.double()).sum(), x64)
    xd = x.to(DEV)
    act = torch.empty(rows, A, device=DEV)
    K.nat.call("sd_bnormal_sample", K.p(xd), K.p(act), rows, A, MIN_STD, MAX_STD, BN_SEED, nz.STREAM_ACT, BN_STEP,
               BN_ROW_OFFSET, 0, K.stream())
    close(act, a64, 1e-5, "the sample the backward differentiates")
    got = K.bnormal_sample_bwd(d_an.to(DEV), xd, act, MIN_STD, MAX_STD, BN_SEED, nz.STREAM_ACT, BN_STEP, BN_ROW_OFFSET)
    torch.cuda.synchronize()
    assert got.shape == (rows, 2 * A)
    close(got, want, 1e-5, "d_logits")
    assert bool(got[:, A:].any()), "the std half takes the eps part of the gradient"

