"""Small conv encoder / decoder stage cases for pinning csrc/conv.hip (every forward, weight-gradient and
input-gradient kernel and the host plans that pick among them) and the stage's row kernels in csrc/poolnorm.hip to a float64 reference at every kind of shape the
Python surface admits, not only the BASELINE stages. Test infrastructure (a plain module: no fixtures, no hooks).

Shared by tests/test_conv_parity_cpu.py (the tie margin, the float32 restatement against float64, mutated references,
the plans against the library's host-only queries) and tests/test_gpu_conv_f64.py (the product against float64).

The reference is plain torch on the CPU in float64: F.pad as oracle/ref_cpu.conv_same pads, F.conv2d, the 2x2 max
pool (as a gather at the window argmax, asserted equal to F.max_pool2d), F.rms_norm over the channels, F.silu, a
nearest upsample for the decoder and autograd for every gradient. It calls nothing from sdreamer.

The four host plans of the direct weight-gradient kernels (direct_plan, direct3_plan, pool_plan, pool3_plan) and the
forward / input-gradient gates are restated here in Python, so every case names the arm it is meant to reach and the
tests notice when a retuned plan moves a case off it.

Index rule: the saved argmax must be EQUAL everywhere, no window excluded. The CPU file enforces, per case, that every
pooling window's top-2 margin in float64 is >= 32 x the case's worst float32-restatement conv-output error; a case
that misses it gets another seed (chosen on the CPU from the reference alone).
"""
import functools
from dataclasses import dataclass, replace

import numpy as np
import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
EPS = 1e-4  # nn.RMSNorm(eps=1e-4)
FWD_TOL, GRAD_TOL = 2e-5, 5e-5  # test_gpu_ops.test_conv_pool_norm's close() tolerances, used as caps
C_SPLIT = 4e-5  # test_gpu_ops.test_conv_backward_bf16x3: per-product split error <= 3 * 2^-17
F32_SLACK = 8.0  # f32 arms: 8 x the float32 restatement's own worst |err| / contraction(|a|, |b|)
FLOOR = dict(fwd=1e-6, dgrad=1e-6, wgrad=1e-5)  # test_conv_backward_bf16x3's absolute floors
MARGIN_FACTOR = 32.0
MAX_SEEDS = 16

# csrc/conv.hip constants
MAX_TAPQ, NW_D, WD_VA, WD_VP, WGRAD_POOL_PIX = 512, 8, 4, 6, 512
WS_REDUCE_BYTES = NW_D * 4 * 64 * 4  # the wave-split plans' end-of-kernel reduction through LDS


# ===================================================================================================== the host plans
def ilog2_exact(v):
    return v.bit_length() - 1 if v > 0 and not v & (v - 1) else -1


def patch_stride(Ci):
    if Ci < 16:
        return (Ci + 2 + 3) // 4 * 4
    c = (Ci + 2 + 15) // 16 * 16
    while c % 64 not in (16, 48):
        c += 16
    return c


def _grid(pl, Nb, H):
    blocks = Nb * (H // pl["R"])
    pl["gy"] = max(1, min(256 // pl["gx"], blocks))
    pl["slabs"] = pl["gy"]
    return pl


def direct_plan(Nb, H, W, Ci, Co, kh, kw, ups=0, pool_pix=0):
    """conv_wgrad_direct<TM, NBW, WS, PL> (f32): dict(R, nbw, gx, gy, slabs, ws, tm, lds) or None"""
    pool = pool_pix > 0
    if ups or Co % 16 or Co > 64 or Ci % 4 or ilog2_exact(W) < 0:
        return None
    pix = pool_pix if pool else 128
    R = 1 if W >= pix else (pix // W if pix // W < H else H)
    if H % R or (R * W) % 4:
        return None
    SA, CP = (Co + 16 if Co % 32 == 0 else Co), patch_stride(Ci)
    PH, PW = R + kh - 1, W + kw - 1
    lds = (R * W * SA + PH * PW * CP) * 4
    if lds > 160 * 1024:
        return None
    if R * W * Co // (16 if pool else 4) > WD_VA * 512 or PH * PW * (Ci // 4) > WD_VP * 512:
        return None
    JB = (kh * kw * Ci + 1 + 15) // 16
    ws = JB <= 7
    nbw = 7 if ws else 2 if JB <= 16 else 4 if JB <= 32 else 7 if JB <= 56 else (10 if Co <= 48 else 7)
    gx = 1 if ws else (JB + NW_D * nbw - 1) // (NW_D * nbw)
    if ws:
        lds = max(lds, WS_REDUCE_BYTES)
    return _grid(dict(R=R, nbw=nbw, gx=gx, ws=ws, tm=Co // 16, lds=lds), Nb, H)


def pool_plan(Nb, H, W, Ci, Co, kh, kw):
    """the pooled-gradient f32 plan: the largest block <= WGRAD_POOL_PIX pixels whose staging fits"""
    if H % 2 or W % 2:
        return None
    pix = WGRAD_POOL_PIX
    while pix >= 128:
        pl = direct_plan(Nb, H, W, Ci, Co, kh, kw, 0, pix)
        if pl and pl["ws"] and pl["nbw"] == 7 and pl["R"] % 2 == 0:
            return pl
        pix //= 2
    return None


def direct3_plan(Nb, H, W, Ci, Co, kh, kw, ups=0):
    """conv_wgrad3_direct<TM, NBW> (split-bf16)"""
    if ups or Co % 4 or Co > 64 or Ci % 4 or Ci < 16 or W < 8 or ilog2_exact(W) < 0 or W > 128:
        return None
    R = 128 // W if 128 // W < H else H
    P = R * W
    if H % R or P % 32:
        return None
    TM, CP = (Co + 15) // 16, patch_stride(Ci)
    PH, PW = R + kh - 1, W + kw - 1
    lds = PH * PW * CP * 4 + TM * 16 * (P + 8) * 2 * 2
    if lds > 160 * 1024 or PH * PW * (Ci // 4) > WD_VP * 512 or (Co // 4) * (P // 4) > 512:
        return None
    JB = (kh * kw * Ci + 1 + 15) // 16
    nmax = 7 if TM <= 3 else 4
    gx = (JB + NW_D * nmax - 1) // (NW_D * nmax)
    need = (JB + NW_D * gx - 1) // (NW_D * gx)
    nbw = 2 if need <= 2 else 4 if need <= 4 else 5 if need <= 5 else 7
    return _grid(dict(R=R, nbw=nbw, gx=gx, ws=False, tm=TM, lds=lds), Nb, H)


def pool3_plan(Nb, H, W, Ci, Co, kh, kw):
    """conv_wgrad3_direct<TM, 7, WS, PL>: the first stage's pooled-gradient split-bf16 plan"""
    if Co % 4 or Co > 64 or Ci % 4 or W < 8 or ilog2_exact(W) < 0 or W > 256 or H % 2:
        return None
    JB = (kh * kw * Ci + 1 + 15) // 16
    if JB > 7:
        return None
    R = 256 // W
    if R < 2 or R % 2 or H % R:
        return None
    P, TM, CP = R * W, (Co + 15) // 16, patch_stride(Ci)
    PH, PW = R + kh - 1, W + kw - 1
    if (Co // 4) * (P // 4) > 512 or PH * PW * (Ci // 4) > WD_VP * 512:
        return None
    lds = PH * PW * CP * 4 + TM * 16 * (P + 8) * 2 * 2
    if lds > 160 * 1024:
        return None
    blocks = Nb * (H // R)
    return dict(R=R, nbw=7, gx=1, gy=min(blocks, 256), slabs=min(blocks, 256), ws=True, tm=TM, lds=lds)


def _tile(Co, va, vb, what):
    return f"{what}<{'128,32' if Co <= 32 else '128,64'}{',VA' if va else ''}{',VB' if vb else ''}>"


def plain_fwd_arm(H, W, Ci, Co, k, ups=0):
    """sd_conv2d_fwd's kernel (weight and input 16-byte aligned, as torch allocates them)"""
    vb = (k * k * Ci) % 4 == 0
    va = Ci % 4 == 0 and vb
    Hg, Wg = H << ups, W << ups
    pow2 = ilog2_exact(Wg) >= 0 and ilog2_exact(Hg * Wg) >= 0
    if va and pow2 and k * k * Ci // 4 <= MAX_TAPQ and Co in (16, 32, 48, 64):
        return f"conv_fwd16<{Co}>"
    return _tile(Co, va, vb, "conv_fwd_kernel")


def fused_fwd_arm(Nb, H, W, Ci, Co, k):
    """K.conv2d_fwd_pool's kernel with CONV6 on, or None where it returns None (the caller then runs two launches)"""
    M, lhw = Nb * H * W, ilog2_exact(H * W)
    if k == 5 and H == W and H % 2 == 0 and lhw >= 0 and M % 128 == 0 and (Co, Ci, W) in ((48, 32, 32), (64, 48, 16)):
        return "conv_fwd6r_direct_pool"
    va = Ci % 4 == 0
    if not va or ilog2_exact(W) < 1 or lhw < 0 or k * k * Ci // 4 > MAX_TAPQ or H % 2 or 128 % (2 * W) or M % 128:
        return None
    if (Co, Ci, W, k) == (48, 32, 32, 5) and H % 4 == 0:
        return "conv_fwd_direct_pool"
    if (Co, Ci, W, k) == (32, 4, 64, 5):
        return "conv_fwd_direct_pool_c4"
    return f"conv_fwd16_pool<{Co}>" if Co in (16, 32, 48, 64) else None


def dgrad_arm(H, W, C, N, k, fast=True):
    """K.conv2d_dgrad's kernel: dOut has C channels, dIn has N"""
    if fast and k == 5 and H == W and H % 16 == 0 and (C, N, W) in ((48, 32, 32), (64, 48, 16)):
        return "conv_dgrad3_direct"
    if (fast and C % 4 == 0 and ilog2_exact(W) >= 0 and ilog2_exact(H * W) >= 0 and k * k * C // 4 <= MAX_TAPQ
            and N in (16, 32, 48, 64)):
        return f"conv_dgrad3<{N}>"
    return plain_fwd_arm(H, W, C, N, k)


def wgrad_arm(Nb, H, W, Ci, Co, k, ups=0, fast=True):
    """K.conv2d_wgrad's kernel"""
    pl = direct3_plan(Nb, H, W, Ci, Co, k, k, ups) if fast else None
    if pl:
        return f"conv_wgrad3_direct<{pl['tm']},{pl['nbw']}>"
    pl = direct_plan(Nb, H, W, Ci, Co, k, k, ups) if Co % 4 == 0 and Ci % 4 == 0 else None
    if pl:
        return f"conv_wgrad_direct<{pl['tm']},{pl['nbw']}{',WS' if pl['ws'] else ''}>"
    tile = _tile(Co, Co % 4 == 0, Ci % 4 == 0, "conv_wgrad_kernel")
    return tile.replace("128,32", "32,128").replace("128,64", "64,64")


def check_plans(nat, Nb, H, W, Ci, Co, k, ups=0):
    """the four plans (and the pooled input gradient's gate) against the library's host-only queries (no launch)"""
    q = nat.fns
    what = (Nb, H, W, Ci, Co, k, ups)
    pl = direct_plan(Nb, H, W, Ci, Co, k, k, ups)
    assert q["sd_conv2d_wgrad_slabs"](Nb, H, W, Ci, Co, k, k, ups, 3) == (pl["slabs"] if pl else 3), what
    pl = direct3_plan(Nb, H, W, Ci, Co, k, k, ups)
    want = pl["slabs"] if pl else nat.SD_ESHAPE
    assert q["sd_conv2d_wgrad_bf16x3_slabs"](Nb, H, W, Ci, Co, k, k, ups) == want, what
    if ups == 0:
        pl = pool_plan(Nb, H, W, Ci, Co, k, k)
        assert q["sd_conv2d_wgrad_pool_slabs"](Nb, H, W, Ci, Co, k, k) == (pl["slabs"] if pl else 0), what
        pl = pool3_plan(Nb, H, W, Ci, Co, k, k)
        assert q["sd_conv2d_wgrad_pool_bf16x3_slabs"](Nb, H, W, Ci, Co, k, k) == (pl["slabs"] if pl else 0), what
        ok = (Co, Ci, k, W) == (32, 3, 5, 64) and H >= 2 and H % 2 == 0
        assert bool(q["sd_conv2d_dgrad_pool_ok"](H, W, Co, Ci, k, k, (k - 1) // 2)) == ok, what


# ===================================================================================================== the cases
@dataclass(frozen=True)
class StageCase:
    """One ConvPoolNormFn call, plain or FiLM (ipc): x (nb, H, W, ci) -> (nb, H/2, W/2, co)."""
    name: str
    ci: int
    co: int
    H: int
    W: int
    k: int
    nb: int
    dx: bool  # the input gradient is wanted
    fwd: str  # the arms the case is meant to reach (stage_arms restates them from the plans)
    wgrad: str
    dgrad: str
    raw: bool = False  # x is the 3-channel image in [0, 1]: the stage (dx) or K.pad_channels (no dx) forms x - 0.5 | 0
    ipc: int = 0  # > 0: the FiLM stage with this many images per context row
    nchw: bool = False
    x3: bool = True  # kernels.WGRAD1_X3
    seed: int = 0

    @property
    def cx(self):  # the channel count the kernels see
        return (self.ci + 3) // 4 * 4 if self.raw else self.ci


@dataclass(frozen=True)
class UpCase:
    """One UpConvFn call (then rms_silu unless `last`): x (nb, H, W, ci) -> (nb, 2H, 2W, co)."""
    name: str
    ci: int
    co: int
    H: int
    W: int
    k: int
    nb: int
    fwd: str
    wgrad: str
    dgrad: str
    last: bool = False
    seed: int = 0


@dataclass(frozen=True)
class KernelCase:
    """One contraction on a kernels.py entry point: op in (fwd, dgrad, wgrad). fwd / wgrad: x (nb, H, W, ci) and
    (nb, H << ups, W << ups, co); dgrad: dOut (nb, H, W, co) -> (nb, H, W, ci)."""
    name: str
    op: str
    ci: int
    co: int
    H: int
    W: int
    k: int
    nb: int
    arm: str  # the f32 arm (fast=False)
    fast: str = ""  # the split-bf16 arm fast=True takes, "" where it takes the f32 one as well
    ups: int = 0
    seed: int = 0


POOL3, POOLF = "conv_wgrad3_direct<{},7,WS,PL>", "conv_wgrad_direct<{},7,WS,PL> R={}"
S = StageCase
STAGE_CASES = [
    # ---- first stage (3 -> 32 padded to 4, W = 64): the pooled weight gradient in both forms, conv_dgrad_pool_k
    S("s1_16x64_dx", 3, 32, 16, 64, 5, 1, True, "conv_fwd_direct_pool_c4", POOL3.format(2), "conv_dgrad_pool_k",
      raw=True),
    S("s1_16x64", 3, 32, 16, 64, 5, 1, False, "conv_fwd_direct_pool_c4", POOL3.format(2), "-", raw=True),
    S("s1_16x64_f32", 3, 32, 16, 64, 5, 1, False, "conv_fwd_direct_pool_c4", POOLF.format(2, 8), "-", raw=True,
      x3=False),
    # H = 18: H * W is no power of two (two launches, generic tiles), 18 % 4 (pool3_plan refuses: the f32 pooled kernel
    # at its smallest block), and conv_dgrad_pool_k's second 16-row tile holds 2 rows
    S("s1_18x64_dx", 3, 32, 18, 64, 5, 1, True, "conv_fwd_kernel<128,32,VA,VB> + pool_rms", POOLF.format(2, 2),
      "conv_dgrad_pool_k", raw=True, nchw=True),
    S("s1_18x64", 3, 32, 18, 64, 5, 1, False, "conv_fwd_kernel<128,32,VA,VB> + pool_rms", POOLF.format(2, 2), "-",
      raw=True),
    S("s1_2x64_dx", 3, 32, 2, 64, 5, 2, True, "conv_fwd_direct_pool_c4", POOLF.format(2, 2), "conv_dgrad_pool_k",
      raw=True),
    # W = 128: no fused forward (a tile holds no row pair), the pooled split kernel at R = 2 rows of 128
    S("s1_4x128", 3, 32, 4, 128, 5, 1, False, "conv_fwd16<32> + pool_rms", POOL3.format(2), "-", raw=True),
    # W = 16: outside conv_dgrad_pool_k, so the image's gradient takes the full-resolution route: pool_rms_bwd, the f32
    # wave-split kernel on the padded input, conv2d_dgrad on the zero-padded weight and the slice back to 3 channels
    S("s1_6x16_dx", 3, 32, 6, 16, 5, 2, True, "conv_fwd_kernel<128,32,VA,VB> + pool_rms", "conv_wgrad_direct<2,7,WS>",
      "conv_fwd_kernel<128,32,VA,VB>", raw=True),
    # ---- 3x3 and 4x4 (even: pad 1 left / 2 right, the input gradient pads 2 / 1)
    S("k3_16_32", 16, 32, 16, 16, 3, 2, True, "conv_fwd16_pool<32>", "conv_wgrad3_direct<2,2>", "conv_dgrad3<16>",
      seed=2),
    S("k4_16_32", 16, 32, 16, 16, 4, 2, True, "conv_fwd16_pool<32>", "conv_wgrad3_direct<2,4>", "conv_dgrad3<16>"),
    S("k4_4_32", 4, 32, 16, 16, 4, 2, True, "conv_fwd16_pool<32>", "conv_wgrad_direct<2,7,WS>",
      "conv_fwd_kernel<128,32,VA,VB>"),
    S("k4_4_32_nodx", 4, 32, 16, 16, 4, 2, False, "conv_fwd16_pool<32>", POOL3.format(2), "-"),
    # ---- Co % 16 != 0
    S("co24", 16, 24, 16, 16, 5, 2, True, "conv_fwd_kernel<128,32,VA,VB> + pool_rms", "conv_wgrad3_direct<2,4>",
      "conv_dgrad3<16>"),
    S("co40", 24, 40, 8, 8, 5, 3, True, "conv_fwd_kernel<128,64,VA,VB> + pool_rms", "conv_wgrad3_direct<3,5>",
      "conv_fwd_kernel<128,32,VA,VB>", nchw=True),
    # ---- Co > 64 / K / 4 > MAX_TAPQ: every fast path refuses
    S("co96", 64, 96, 8, 8, 5, 2, True, "conv_fwd_kernel<128,64,VA,VB> + pool_rms", "conv_wgrad_kernel<64,64,VA,VB>",
      "conv_fwd_kernel<128,64,VA,VB>"),
    S("co128", 96, 128, 4, 4, 5, 3, True, "conv_fwd_kernel<128,64,VA,VB> + pool_rms", "conv_wgrad_kernel<64,64,VA,VB>",
      "conv_fwd_kernel<128,64,VA,VB>", nchw=True),
    # ---- non-square, not a power of two, odd
    S("h16_w32", 16, 32, 16, 32, 5, 2, True, "conv_fwd16_pool<32>", "conv_wgrad3_direct<2,4>", "conv_dgrad3<16>",
      seed=1),
    S("h32_w16", 16, 32, 32, 16, 5, 2, True, "conv_fwd16_pool<32>", "conv_wgrad3_direct<2,4>", "conv_dgrad3<16>",
      nchw=True, seed=4),
    S("hw24", 16, 32, 24, 24, 5, 1, True, "conv_fwd_kernel<128,32,VA,VB> + pool_rms", "conv_wgrad_kernel<32,128,VA,VB>",
      "conv_fwd_kernel<128,32,VA,VB>", seed=2),
    S("hw21", 16, 32, 21, 21, 5, 2, True, "conv_fwd_kernel<128,32,VA,VB> + pool_rms", "conv_wgrad_kernel<32,128,VA,VB>",
      "conv_fwd_kernel<128,32,VA,VB>", nchw=True),
    S("hw21_c4", 4, 32, 21, 21, 5, 2, True, "conv_fwd_kernel<128,32,VA,VB> + pool_rms",
      "conv_wgrad_kernel<32,128,VA,VB>",
      "conv_fwd_kernel<128,32,VA,VB>", seed=1),
    S("h21_w16", 16, 32, 21, 16, 5, 1, True, "conv_fwd_kernel<128,32,VA,VB> + pool_rms",
      "conv_wgrad_kernel<32,128,VA,VB>",
      "conv_fwd_kernel<128,32,VA,VB>"),
    # ---- tiny images
    S("hw4_nb5", 64, 64, 4, 4, 5, 5, True, "conv_fwd16<64> + pool_rms", "conv_wgrad_direct<4,7> gx=2",
      "conv_dgrad3<64>"),
    S("hw2_nb3", 64, 64, 2, 2, 5, 3, True, "conv_fwd16<64> + pool_rms", "conv_wgrad_direct<4,7> gx=2",
      "conv_dgrad3<64>"),
    S("hw2_nb32", 64, 64, 2, 2, 5, 32, True, "conv_fwd16_pool<64>", "conv_wgrad_direct<4,7> gx=2", "conv_dgrad3<64>",
      nchw=True, seed=2),
    # ---- narrow Ci in a non-first stage (the f32 wave-split plan; without dx the pooled plans take it)
    S("ci8_k3", 8, 16, 16, 16, 3, 2, True, "conv_fwd16_pool<16>", "conv_wgrad_direct<1,7,WS>",
      "conv_fwd_kernel<128,32,VA,VB>"),
    S("ci8_k3_nodx", 8, 16, 16, 16, 3, 2, False, "conv_fwd16_pool<16>", POOL3.format(1), "-"),
    S("ci12_k3", 12, 16, 8, 8, 3, 2, True, "conv_fwd16_pool<16>", "conv_wgrad_direct<1,7,WS>",
      "conv_fwd_kernel<128,32,VA,VB>"),
    # ---- the f32 pooled kernel at 1, 3 and 4 blocks of 16 output channels (the first stage has 2)
    S("pl_f32_tm1", 4, 16, 4, 4, 3, 2, False, "conv_fwd16<16> + pool_rms", POOLF.format(1, 4), "-", x3=False),
    S("pl_f32_tm3", 4, 48, 4, 4, 3, 3, False, "conv_fwd16<48> + pool_rms", POOLF.format(3, 4), "-", x3=False),
    S("pl_f32_tm4", 4, 64, 4, 4, 3, 1, False, "conv_fwd16<64> + pool_rms", POOLF.format(4, 4), "-", x3=False),
    # ---- anchors: the BASELINE stages at Nb 1 (64 -> 64 at 8 x 8: 64 pixels, half a tile; Nb 3: a ragged second tile)
    S("a_32_48", 32, 48, 32, 32, 5, 1, True, "conv_fwd6r_direct_pool", "conv_wgrad3_direct<3,7>", "conv_dgrad3_direct"),
    S("a_48_64", 48, 64, 16, 16, 5, 1, True, "conv_fwd6r_direct_pool", "conv_wgrad3_direct<4,4> gx=3",
      "conv_dgrad3_direct", seed=2),
    S("a_64_64_nb1", 64, 64, 8, 8, 5, 1, True, "conv_fwd16<64> + pool_rms", "conv_wgrad3_direct<4,4> gx=4",
      "conv_dgrad3<64>",
      nchw=True, seed=1),
    S("a_64_64_nb3", 64, 64, 8, 8, 5, 3, True, "conv_fwd16<64> + pool_rms", "conv_wgrad3_direct<4,4> gx=4",
      "conv_dgrad3<64>",
      nchw=True, seed=2),
    # ---- FiLM: ipc = 2 and ipc = Nb, on the fused kernel and on the two-launch fall-back (Co = 24, odd size)
    S("film_fused", 16, 32, 8, 8, 5, 4, True, "conv_fwd16_pool<32>", "conv_wgrad3_direct<2,4>", "conv_dgrad3<16>",
      ipc=2),
    S("film_fused_row", 16, 32, 8, 8, 5, 4, True, "conv_fwd16_pool<32>", "conv_wgrad3_direct<2,4>",
      "conv_dgrad3<16>", ipc=4,
      nchw=True),
    # a 128-pixel tile spans two context rows
    S("film_ipc1", 16, 32, 8, 8, 5, 4, True, "conv_fwd16_pool<32>", "conv_wgrad3_direct<2,4>", "conv_dgrad3<16>",
      ipc=1),
    S("film_co24", 16, 24, 8, 8, 5, 4, True, "conv_fwd_kernel<128,32,VA,VB> + pool_rms", "conv_wgrad3_direct<2,4>",
      "conv_dgrad3<16>", ipc=2),
    S("film_hw7", 16, 24, 7, 7, 3, 4, True, "conv_fwd_kernel<128,32,VA,VB> + pool_rms",
      "conv_wgrad_kernel<32,128,VA,VB>",
      "conv_fwd_kernel<128,32,VA,VB>", ipc=4, nchw=True),
    S("film_s1", 3, 32, 16, 64, 5, 2, False, "conv_fwd_direct_pool_c4", POOL3.format(2), "-", raw=True, ipc=2),
]
U = UpCase
UP_CASES = [
    U("up_64_48", 64, 48, 4, 4, 5, 2, "conv_fwd16<48>", "conv_wgrad_kernel<64,64,VA,VB>", "conv_dgrad3<64>"),
    U("up_last", 32, 3, 8, 8, 5, 3, "conv_fwd_kernel<128,32,VA,VB>", "conv_wgrad_kernel<32,128,VB>",
      "conv_fwd_kernel<128,32>",
      last=True),
    U("up_k4", 16, 16, 4, 4, 4, 2, "conv_fwd16<16>", "conv_wgrad_kernel<32,128,VA,VB>", "conv_dgrad3<16>"),
    U("up_4x8", 16, 32, 4, 8, 5, 2, "conv_fwd16<32>", "conv_wgrad_kernel<32,128,VA,VB>", "conv_dgrad3<16>"),
    U("up_128_64", 128, 64, 4, 4, 5, 2, "conv_fwd_kernel<128,64,VA,VB>", "conv_wgrad_kernel<64,64,VA,VB>",
      "conv_fwd_kernel<128,64,VA,VB>"),
    U("up_3x5_k3", 8, 24, 3, 5, 3, 2, "conv_fwd_kernel<128,32,VA,VB>", "conv_wgrad_kernel<32,128,VA,VB>",
      "conv_fwd_kernel<128,32,VA,VB>"),
]
KC = KernelCase
KERNEL_CASES = [
    # ---- conv_wgrad_direct (f32): NBW 2 / 4 / 7 / 10 and WS, TM 1-4, gx > 1; the split-bf16 tests' yardstick
    KC("wg_ws_tm1", "wgrad", 8, 16, 16, 16, 3, 2, "conv_wgrad_direct<1,7,WS>"),
    KC("wg_ws_tiny", "wgrad", 4, 16, 4, 4, 3, 2, "conv_wgrad_direct<1,7,WS>"),  # staging < the WS reduction's 8 KiB
    KC("wg_nbw2_tm2", "wgrad", 16, 32, 8, 8, 3, 3, "conv_wgrad_direct<2,2>", "conv_wgrad3_direct<2,2>"),
    KC("wg_nbw4_tm3", "wgrad", 16, 48, 8, 8, 5, 2, "conv_wgrad_direct<3,4>", "conv_wgrad3_direct<3,4>"),
    KC("wg_nbw7_tm4", "wgrad", 32, 64, 4, 4, 5, 3, "conv_wgrad_direct<4,7>"),
    KC("wg_nbw10_tm1", "wgrad", 48, 16, 8, 8, 5, 2, "conv_wgrad_direct<1,10>", "conv_wgrad3_direct<1,5> gx=2"),
    KC("wg_nbw10_gx2", "wgrad", 64, 48, 4, 4, 5, 2, "conv_wgrad_direct<3,10> gx=2"),
    KC("wg_nbw7_gx2", "wgrad", 64, 64, 4, 4, 5, 5, "conv_wgrad_direct<4,7> gx=2"),
    KC("wg_k4_h12", "wgrad", 16, 32, 12, 8, 4, 1, "conv_wgrad_direct<2,4>", "conv_wgrad3_direct<2,4>"),  # R = 12 of 16
    # one image row per block
    KC("wg_w128_r1", "wgrad", 16, 32, 3, 128, 3, 1, "conv_wgrad_direct<2,2>", "conv_wgrad3_direct<2,2>"),
    # the rest of the rungs the plans can reach (test_conv_parity_cpu enumerates them), at the smallest shape of each
    KC("wg_tm1_nbw2", "wgrad", 16, 16, 8, 8, 3, 2, "conv_wgrad_direct<1,2>", "conv_wgrad3_direct<1,2>"),
    KC("wg_tm1_nbw4", "wgrad", 32, 16, 8, 8, 3, 3, "conv_wgrad_direct<1,4>", "conv_wgrad3_direct<1,4>"),
    KC("wg_tm1_nbw7", "wgrad", 32, 16, 8, 8, 5, 1, "conv_wgrad_direct<1,7>", "conv_wgrad3_direct<1,7>"),
    KC("wg_tm2_nbw7", "wgrad", 24, 32, 8, 8, 5, 2, "conv_wgrad_direct<2,7>", "conv_wgrad3_direct<2,5>"),
    KC("wg_tm2_nbw10", "wgrad", 64, 32, 8, 8, 5, 1, "conv_wgrad_direct<2,10> gx=2", "conv_wgrad3_direct<2,7> gx=2"),
    KC("wg_tm3_nbw2", "wgrad", 16, 48, 8, 8, 3, 2, "conv_wgrad_direct<3,2>", "conv_wgrad3_direct<3,2>"),
    KC("wg_tm3_nbw7", "wgrad", 32, 48, 8, 8, 5, 1, "conv_wgrad_direct<3,7>", "conv_wgrad3_direct<3,7>"),
    KC("wg_tm4_nbw2", "wgrad", 16, 64, 8, 8, 3, 3, "conv_wgrad_direct<4,2>", "conv_wgrad3_direct<4,2>"),
    KC("wg_tm4_nbw4", "wgrad", 32, 64, 8, 8, 3, 1, "conv_wgrad_direct<4,4>", "conv_wgrad3_direct<4,4>"),
    KC("wg_ws_tm3", "wgrad", 4, 48, 4, 4, 3, 2, "conv_wgrad_direct<3,7,WS>"),
    KC("wg_ws_tm4", "wgrad", 4, 64, 4, 4, 3, 3, "conv_wgrad_direct<4,7,WS>"),
    # 260 row blocks over 256 workgroup rows: four workgroups take a second block (prefetched), the others do not
    KC("wg_nb260", "wgrad", 16, 16, 8, 8, 3, 260, "conv_wgrad_direct<1,2>", "conv_wgrad3_direct<1,2>"),
    KC("wg_ups_co3", "wgrad", 16, 3, 4, 4, 5, 2, "conv_wgrad_kernel<32,128,VB>", ups=1),
    # the four VA / VB forms of the split-K tiles
    KC("wg_ci3", "wgrad", 3, 16, 6, 5, 5, 2, "conv_wgrad_kernel<32,128,VA>"),
    KC("wg_ci3_co3", "wgrad", 3, 3, 6, 5, 4, 2, "conv_wgrad_kernel<32,128>"),
    KC("wg_co40_ksplit", "wgrad", 8, 40, 70, 64, 3, 2, "conv_wgrad_kernel<64,64,VA,VB>"),  # 8960 pixels: two k slabs
    # ---- the input gradient on the f32 forward kernels (flipped weight), and the split arm where one takes the shape
    KC("dg_k4_16", "dgrad", 16, 32, 8, 8, 4, 2, "conv_fwd16<16>", "conv_dgrad3<16>"),
    KC("dg_k3_48", "dgrad", 48, 24, 8, 8, 3, 2, "conv_fwd16<48>", "conv_dgrad3<48>"),
    KC("dg_ci24", "dgrad", 24, 40, 8, 8, 5, 3, "conv_fwd_kernel<128,32,VA,VB>"),
    KC("dg_h6", "dgrad", 32, 16, 6, 8, 5, 1, "conv_fwd_kernel<128,32,VA,VB>"),
    KC("fw_ci3_k4", "fwd", 3, 32, 6, 5, 4, 2, "conv_fwd_kernel<128,32,VB>"),  # K % 4 == 0 with Ci % 4 != 0
    KC("fw_ci3_k5", "fwd", 3, 40, 6, 5, 5, 2, "conv_fwd_kernel<128,64>"),
] + [
    # ---- sd_conv2d_fwd with and without the upsample at Co 3 / 16 / 24 / 96
    KC(f"fw_co{co}_ups{u}", "fwd", 16, co, 4, 8, k, 2,
       f"conv_fwd16<{co}>" if co == 16 else _tile(co, True, True, "conv_fwd_kernel"), ups=u)
    for u in (0, 1) for co, k in ((3, 5), (16, 4), (24, 3), (96, 5))
]
STAGE = {c.name: c for c in STAGE_CASES}
UP = {c.name: c for c in UP_CASES}
KERNEL = {c.name: c for c in KERNEL_CASES}
assert len(STAGE) == len(STAGE_CASES) and len(UP) == len(UP_CASES) and len(KERNEL) == len(KERNEL_CASES)


def pooled_route(c):
    """ops.ConvPoolNormFn.backward: the stage's backward runs from the pooled gradient (pool_rms_bwd_compact)"""
    pp = pool_plan(c.nb, c.H, c.W, c.cx, c.co, c.k, c.k)
    dgp = (c.co, c.ci, c.k, c.W) == (32, 3, 5, 64) and c.H >= 2 and c.H % 2 == 0  # sd_conv2d_dgrad_pool_ok
    return bool(pp) and ((c.dx and c.raw and dgp) or not c.dx)


def stage_arms(c):
    """(fwd, wgrad, dgrad) a default ConvPoolNormFn call reaches, from the restated plans and gates"""
    fused = fused_fwd_arm(c.nb, c.H, c.W, c.cx, c.co, c.k)
    fwd = fused or plain_fwd_arm(c.H, c.W, c.cx, c.co, c.k) + " + pool_rms"
    if pooled_route(c):
        p3 = pool3_plan(c.nb, c.H, c.W, c.cx, c.co, c.k, c.k) if c.x3 else None
        pf = pool_plan(c.nb, c.H, c.W, c.cx, c.co, c.k, c.k)
        wg = POOL3.format(p3["tm"]) if p3 else POOLF.format(pf["tm"], pf["R"])
        return fwd, wg, "conv_dgrad_pool_k" if c.dx else "-"
    wg = wgrad_arm(c.nb, c.H, c.W, c.cx, c.co, c.k)
    pl = direct3_plan(c.nb, c.H, c.W, c.cx, c.co, c.k, c.k) or direct_plan(c.nb, c.H, c.W, c.cx, c.co, c.k, c.k)
    if pl and pl["gx"] > 1:
        wg += f" gx={pl['gx']}"
    return fwd, wg, dgrad_arm(c.H, c.W, c.co, c.cx, c.k) if c.dx else "-"


def up_arms(c):
    return (plain_fwd_arm(c.H, c.W, c.ci, c.co, c.k, 1), wgrad_arm(c.nb, c.H, c.W, c.ci, c.co, c.k, 1),
            dgrad_arm(2 * c.H, 2 * c.W, c.co, c.ci, c.k))


def kernel_arms(c):
    """(the f32 arm, the split-bf16 arm or "")"""
    def gx(name, pl):
        return name + (f" gx={pl['gx']}" if pl and pl["gx"] > 1 else "")
    if c.op == "fwd":
        return plain_fwd_arm(c.H, c.W, c.ci, c.co, c.k, c.ups), ""
    if c.op == "dgrad":
        slow, fast = dgrad_arm(c.H, c.W, c.co, c.ci, c.k, False), dgrad_arm(c.H, c.W, c.co, c.ci, c.k, True)
        return slow, fast if fast != slow else ""
    args = (c.nb, c.H, c.W, c.ci, c.co, c.k, c.k, c.ups)
    slow = gx(wgrad_arm(c.nb, c.H, c.W, c.ci, c.co, c.k, c.ups, False), direct_plan(*args))
    fast = gx(wgrad_arm(c.nb, c.H, c.W, c.ci, c.co, c.k, c.ups, True), direct3_plan(*args))
    return slow, fast if direct3_plan(*args) else ""


# ===================================================================================================== inputs
def _gen(c, salt):
    return torch.Generator().manual_seed(1000 * c.seed + salt)


@functools.lru_cache(maxsize=None)
def stage_inputs(c):
    """x (NHWC), w (Co, Ci, k, k), b, nw, gamma, beta (FiLM rows or None), dy (the output's shape); CPU float32"""
    g = _gen(c, 1)
    x = torch.rand(c.nb, c.H, c.W, c.ci, generator=g) - (0.0 if c.raw else 0.5)
    w = torch.randn(c.co, c.ci, c.k, c.k, generator=g) / (c.ci * c.k * c.k) ** 0.5
    b = 0.1 * torch.randn(c.co, generator=g)
    nw = 1 + 0.1 * torch.randn(c.co, generator=g)
    gamma = beta = None
    if c.ipc:
        gamma = 1 + 0.3 * torch.randn(c.nb // c.ipc, c.co, generator=g)
        beta = 0.3 * torch.randn(c.nb // c.ipc, c.co, generator=g)
    Ho, Wo = c.H // 2, c.W // 2
    dy = torch.randn((c.nb, c.co * Ho * Wo) if c.nchw else (c.nb, Ho, Wo, c.co), generator=g)
    return x, w, b, nw, gamma, beta, dy


@functools.lru_cache(maxsize=None)
def up_inputs(c):
    g = _gen(c, 2)
    x = torch.randn(c.nb, c.H, c.W, c.ci, generator=g)
    w = torch.randn(c.co, c.ci, c.k, c.k, generator=g) / (c.ci * c.k * c.k) ** 0.5
    b = 0.1 * torch.randn(c.co, generator=g)
    nw = 1 + 0.1 * torch.randn(c.co, generator=g)
    dy = torch.randn(c.nb, 2 * c.H, 2 * c.W, c.co, generator=g)
    return x, w, b, nw, dy


@functools.lru_cache(maxsize=None)
def kernel_inputs(c):
    """x (nb, H, W, ci), w (co, ci, k, k), dout (nb, H << ups, W << ups, co); CPU float32"""
    g = _gen(c, 3)
    x = torch.rand(c.nb, c.H, c.W, c.ci, generator=g) - 0.5
    w = torch.randn(c.co, c.ci, c.k, c.k, generator=g) / (c.ci * c.k * c.k) ** 0.5
    dout = torch.randn(c.nb, c.H << c.ups, c.W << c.ups, c.co, generator=g)
    return x, w, dout


# ===================================================================================================== the reference
MUTANTS = ("pad", "route", "dw_rows", "odd_edge", "ups")


def conv_same(x, w, b, mut=None):
    """oracle/ref_cpu.conv_same (NCHW). mut == "pad": an even kernel's two pad sides swapped; an odd kernel's
    right-most tap column does not see the image's last column (a `xx < W - 1` bound)"""
    k = w.shape[-1]
    lo, hi = (k - 1) // 2, (k - 1) - (k - 1) // 2
    if mut == "pad" and k % 2 == 0:
        lo, hi = hi, lo
    y = F.conv2d(F.pad(x, [lo, hi, lo, hi]), w, b)
    if mut == "pad" and k % 2:
        xl, wl = torch.zeros_like(x), torch.zeros_like(w)
        xl[..., -1] = x[..., -1]
        wl[..., -1] = w[..., -1]
        y = y - F.conv2d(F.pad(xl, [lo, hi, lo, hi]), wl)
    return y


def upsample2(x, mut=None):
    """nearest 2x (NCHW) as a gather at yy >> 1, xx >> 1 (asserted equal to F.interpolate in the CPU file);
    mut == "ups": the source index is min(xx, W - 1) instead"""
    H, W = x.shape[-2:]
    iy, ix = torch.arange(2 * H) >> 1, torch.arange(2 * W) >> 1
    if mut == "ups":
        iy, ix = torch.arange(2 * H).clamp(max=H - 1), torch.arange(2 * W).clamp(max=W - 1)
    return x[..., iy, :][..., ix]


def _odd_edge_hook(H, W):
    """the conv gradient's row / column that MaxPool2d(2) dropped holds its neighbour's values instead of zeros"""
    def hook(g):
        g = g.clone()
        if H % 2:
            g[:, :, H - 1, :] = g[:, :, H - 2, :]
        if W % 2:
            g[:, :, :, W - 1] = g[:, :, :, W - 2]
        return g
    return hook


def _np(t):
    return t.detach().numpy().astype(np.float64)


def run_stage_ref(c, dtype=F64, mut=None):
    return _stage_ref_cached(c, dtype) if mut is None else _stage_ref(c, dtype, mut)


@functools.lru_cache(maxsize=None)
def _stage_ref_cached(c, dtype):
    return _stage_ref(c, dtype, None)


def _stage_ref(c, dtype, mut):
    """The stage in `dtype`: y (the product's output layout), amax (nb, Ho, Wo, co) as window position 2 dy + dx, the
    conv output and every window's top-2 margin, and the gradients of <y, dy>: dx (NHWC), dw (Co, Ci, k, k), db, dnw,
    dgamma, dbeta."""
    # copies: the cached inputs stay leaves that require no gradient
    x, w, b, nw, gamma, beta, dy = (None if t is None else t.clone().to(dtype) for t in stage_inputs(c))
    leaves = dict(x=x, w=w, b=b, nw=nw)
    if c.ipc:
        leaves.update(gamma=gamma, beta=beta)
    for t in leaves.values():
        t.requires_grad_(True)
    xin = (x - 0.5) if c.raw else x
    conv = conv_same(xin.permute(0, 3, 1, 2), w, b, mut)
    if mut == "odd_edge":
        conv.register_hook(_odd_edge_hook(c.H, c.W))
    Ho, Wo = c.H // 2, c.W // 2
    win = conv[:, :, :2 * Ho, :2 * Wo].reshape(c.nb, c.co, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5)
    win = win.reshape(c.nb, c.co, Ho, Wo, 4)
    am = win.detach().argmax(-1, keepdim=True)
    pooled = win.gather(-1, am).squeeze(-1)
    assert torch.equal(pooled.detach(), F.max_pool2d(conv.detach(), 2, 2))
    if mut == "route":  # the value stays, the last pooled column's gradient goes to window position 0
        am_b = am.clone()
        am_b[:, :, :, Wo - 1] = 0
        wrong = win.gather(-1, am_b).squeeze(-1)
        pooled = pooled.detach() + wrong - wrong.detach()
    z = F.rms_norm(pooled.permute(0, 2, 3, 1), (c.co,), nw, EPS)
    if c.ipc:
        rows = torch.arange(c.nb) // c.ipc
        z = gamma[rows][:, None, None, :] * z + beta[rows][:, None, None, :]
    y = F.silu(z)
    if c.nchw:
        y = y.permute(0, 3, 1, 2).reshape(c.nb, -1)
    gr = torch.autograd.grad((y * dy).sum(), list(leaves.values()))
    out = dict(y=_np(y), amax=am.squeeze(-1).permute(0, 2, 3, 1).numpy().astype(np.uint8),
               conv=_np(conv.permute(0, 2, 3, 1)))
    top2 = win.detach().topk(2, -1).values
    out["margin"] = float((top2[..., 0] - top2[..., 1]).min())
    for name, g in zip(leaves, gr):
        out["d" + name] = _np(g)
    if mut == "dw_rows":
        out["dw"][16 * (c.co // 16):] = 0.0
    return out


def run_up_ref(c, dtype=F64, mut=None):
    return _up_ref_cached(c, dtype) if mut is None else _up_ref(c, dtype, mut)


@functools.lru_cache(maxsize=None)
def _up_ref_cached(c, dtype):
    return _up_ref(c, dtype, None)


def _up_ref(c, dtype, mut):
    """Upsample(2, nearest) -> Conv2dSamePad (-> RMSNorm2D -> SiLU unless the decoder's last layer), NHWC outputs"""
    x, w, b, nw, dy = (t.clone().to(dtype) for t in up_inputs(c))
    leaves = dict(x=x, w=w, b=b) if c.last else dict(x=x, w=w, b=b, nw=nw)
    for t in leaves.values():
        t.requires_grad_(True)
    y = conv_same(upsample2(x.permute(0, 3, 1, 2), mut), w, b, mut).permute(0, 2, 3, 1)
    if not c.last:
        y = F.silu(F.rms_norm(y, (c.co,), nw, EPS))
    gr = torch.autograd.grad((y * dy).sum(), list(leaves.values()))
    out = dict(y=_np(y))
    for name, g in zip(leaves, gr):
        out["d" + name] = _np(g)
    if mut == "dw_rows":
        out["dw"][16 * (c.co // 16):] = 0.0
    return out


def _contract(c, x, w, dout):
    """the case's contraction in the tensors' dtype, in the product's layout: fwd (nb, Hg, Wg, co); dgrad
    (nb, H, W, ci); wgrad (co, k * k * ci + 1) = [dW as (ky, kx, ci) | db]"""
    xc = x.permute(0, 3, 1, 2)
    if c.op == "fwd":
        return conv_same(upsample2(xc) if c.ups else xc, w, None).permute(0, 2, 3, 1)
    xc, w = xc.clone().requires_grad_(True), w.clone().requires_grad_(True)
    b = torch.zeros(c.co, dtype=x.dtype, requires_grad=True)
    y = conv_same(upsample2(xc) if c.ups else xc, w, b)
    gx, gw, gb = torch.autograd.grad((y * dout.permute(0, 3, 1, 2)).sum(), [xc, w, b])
    if c.op == "dgrad":
        return gx.permute(0, 2, 3, 1)
    return torch.cat([gw.permute(0, 2, 3, 1).reshape(c.co, -1), gb[:, None]], 1)


@functools.lru_cache(maxsize=None)
def run_kernel_ref(c):
    """ref (float64), mag = the same contraction on |operands| (float64), and rho32 = the float32 torch restatement's
    worst |err| / mag over the elements: the f32 arms' bound is F32_SLACK * rho32 * mag + floor"""
    x, w, dout = kernel_inputs(c)
    ref = _contract(c, x.double(), w.double(), dout.double())
    mag = _contract(c, x.double().abs(), w.double().abs(), dout.double().abs())
    r32 = _contract(c, x, w, dout).double()
    rho = float(((r32 - ref).abs() / mag.clamp_min(1e-300)).max())
    return dict(ref=_np(ref), mag=_np(mag), r32=_np(r32), rho32=rho)


# ===================================================================================================== comparisons
def _close(got, ref, tol):
    """test_gpu_ops.close(): (max |got - ref|, the bound tol * max(max |ref|, 1)); the error is inf for a NaN"""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    e = np.abs(np.asarray(got, np.float64) - ref)
    err = float(np.nan_to_num(e, nan=np.inf, posinf=np.inf).max()) if e.size else 0.0
    return err, tol * max(float(np.abs(ref).max()) if e.size else 0.0, 1.0)


def stage_errors(got, ref):
    """name -> (error, bound) over the tensors both hold (y at FWD_TOL, gradients at GRAD_TOL), and the argmax count"""
    out = {k: _close(got[k], ref[k], FWD_TOL if k == "y" else GRAD_TOL)
           for k in ("y", "dx", "dw", "db", "dnw", "dgamma", "dbeta") if k in ref and k in got}
    if "amax" in ref:
        assert got["amax"].shape == ref["amax"].shape
        out["amax"] = (int((got["amax"] != ref["amax"]).sum()), 0)
    return out


def compare_stage(got, ref, what="", need=()):
    """every tensor of `ref` that `got` holds within its cap and the argmax equal everywhere; `need` must be held"""
    missing = [k for k in need if k not in got]
    assert not missing, f"{what}: no {missing}"
    err = stage_errors(got, ref)
    bad = [f"{k}: error {e:.3g} > {bnd:.3g}" if k != "amax" else f"{e} argmax entries differ"
           for k, (e, bnd) in err.items() if not e <= bnd]
    assert not bad, f"{what}: " + "; ".join(bad)
    return err


def kernel_bound(kr, op, c_rel):
    return c_rel * kr["mag"] + FLOOR[op]


def compare_kernel(got, kr, op, c_rel, what=""):
    """|got - ref| <= c_rel * contraction(|a|, |b|) + floor elementwise; returns the worst |err| / contraction"""
    got = np.asarray(got, np.float64)
    assert got.shape == kr["ref"].shape, (got.shape, kr["ref"].shape)
    e = np.nan_to_num(np.abs(got - kr["ref"]), nan=np.inf)
    over = e - kernel_bound(kr, op, c_rel)
    rho = float((e / np.maximum(kr["mag"], 1e-300)).max())
    assert over.max() <= 0, (f"{what}: |err| exceeds {c_rel:.3g} * contraction(|a|, |b|) + {FLOOR[op]} by "
                             f"{over.max():.3g} (worst ratio {rho:.3g})")
    return rho


def with_seed(c, seed):
    return replace(c, seed=seed)
