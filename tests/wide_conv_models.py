"""Wide conv encoder stage cases (a stage width above 128 channels: model.depth > 32, the reference's h3_wider_cnn
control at depth 77 has stages 154 / 231 / 308 / 308) on tests/conv_models.py's reference, inputs and comparisons.
Test infrastructure (a plain module: no fixtures, no hooks), shared by tests/test_wide_conv_cpu.py (the tie margin, the
float32 restatement, mutated references, the host-only queries) and tests/test_gpu_wide_conv_f64.py (the product).

What a wide stage runs: the exact-f32 generic forward tiles (conv_fwd_kernel), the wide row kernels
(sd_pool_rms_wide_fwd / _bwd and their FiLM forms: a wave per pooled pixel), the full-resolution backward route, and
the two N-tiled split-bf16 contractions (sd_conv2d_dgrad_wide3 / sd_conv2d_wgrad_wide3: 128 x 64 tiles, K in 32-deep
steps, bwd-weight in pixel slabs). With SDREAMER_FAST_GEMM=0 the contractions stay on the f32 tiles.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import conv_models as cm

WIDE_MIN, WIDE_MAX = 128, 512  # kernels.WIDE_ROWS_MIN / WIDE_ROWS_MAX (the CPU file ties them)
BM, BN, BK = 128, 64, 32  # the wide contractions' tile
WGRAD_MIN_CI = 64  # SD_WIDE3_WGRAD_MIN_CI: below it (a first stage) the bwd-weight stays on the f32 tiles
DGRAD, WGRAD = "conv_dgrad_wide3", "conv_wgrad_wide3"

S, KC = cm.StageCase, cm.KernelCase


def _fwd(H, W, cx, co, k):
    return cm.plain_fwd_arm(H, W, cx, co, k) + " + pool_rms_wide"


def _wgrad(nb, H, W, cx, co, k, fast=True):
    return WGRAD if fast and wgrad_takes(cx, co) else cm.wgrad_arm(nb, H, W, cx, co, k, 0, False)


def wide_takes(ci, co):
    """the wide arms' gate, as kernels.conv2d_dgrad / conv2d_wgrad apply it after every older fast arm has refused"""
    return max(ci, co) > WIDE_MIN


def wgrad_takes(ci, co):
    return wide_takes(ci, co) and ci >= WGRAD_MIN_CI


def _stage(name, ci, co, H, W, k, nb, dx=True, seed=0, **kw):
    cx = (ci + 3) // 4 * 4 if kw.get("raw") else ci
    return S(name, ci, co, H, W, k, nb, dx, _fwd(H, W, cx, co, k), _wgrad(nb, H, W, cx, co, k), DGRAD if dx else "-",
             seed=seed, **kw)


# the smallest shapes that reach every new path (the seeds: the first meeting the tie-margin rule, re-derived on the CPU)
STAGE_CASES = [
    _stage("w_s1_dx", 3, 154, 8, 8, 5, 2, raw=True),  # the image's gradient: the full route on the padded weight
    _stage("w_154_231", 154, 231, 8, 8, 5, 2, seed=1),
    _stage("w_231_308", 231, 308, 4, 4, 5, 3, nchw=True),
    _stage("w_308_308", 308, 308, 2, 2, 5, 2, nchw=True),
    _stage("w_128_129", 128, 129, 4, 4, 5, 2),  # the first width above the narrow kernels' limit
    _stage("w_96_512", 96, 512, 4, 4, 5, 2, seed=3),  # the cap
    _stage("w_film", 130, 132, 4, 4, 5, 4, ipc=2),
    _stage("w_odd_hw", 154, 231, 6, 10, 3, 3, seed=14),  # odd pooled edge, ragged M tile
]
STAGE = {c.name: c for c in STAGE_CASES}


def _kernel(name, op, ci, co, H, W, k, nb, seed=0):
    probe = KC(name, op, ci, co, H, W, k, nb, "")
    fast = DGRAD if op == "dgrad" else WGRAD if wgrad_takes(ci, co) else ""
    return KC(name, op, ci, co, H, W, k, nb, cm.kernel_arms(probe)[0], fast, seed=seed)


# dgrad: dOut (nb, H, W, co) -> dIn (nb, H, W, ci): M = nb H W, N = ci, K = k k co. wgrad: M = co, N = k k ci + 1,
# K = nb H W pixels. The four depth-77 stages at the small images above (the first stage's operands are the
# channel-padded image's), and the tails the tiles mask.
KERNEL_CASES = [
    _kernel("kd_s1", "dgrad", 4, 154, 8, 8, 5, 2),  # K = 3850: no multiple of 32 nor of 4; N = 4
    _kernel("kd_154_231", "dgrad", 154, 231, 8, 8, 5, 2),  # N = 154 = 2 * 64 + 26
    _kernel("kd_231_308", "dgrad", 231, 308, 4, 4, 5, 3),  # N = 231 = 3 * 64 + 39, M = 48, float4 dOut loads
    _kernel("kd_308_308", "dgrad", 308, 308, 2, 2, 5, 2),
    _kernel("kd_m_tail", "dgrad", 154, 231, 6, 10, 3, 3),  # M = 180 = 128 + 52
    _kernel("kw_s1", "wgrad", 4, 154, 8, 8, 5, 2),  # Ci < 64: stays on the f32 tiles
    _kernel("kw_64_154", "wgrad", 64, 154, 4, 4, 3, 2),  # the smallest Ci taken; M = 154 = 128 + 26, N = 577 = 9 * 64 + 1
    _kernel("kw_154_231", "wgrad", 154, 231, 8, 8, 5, 2),  # N = 3851
    _kernel("kw_231_308", "wgrad", 231, 308, 4, 4, 5, 3),  # K = 48 pixels
    _kernel("kw_308_308", "wgrad", 308, 308, 2, 2, 5, 2),  # K = 8 pixels
    _kernel("kw_slabs", "wgrad", 154, 231, 6, 10, 3, 3),  # K = 180 pixels: three slabs of 64, 64, 52 when forced
]
KERNEL = {c.name: c for c in KERNEL_CASES}
FORCED_SLABS = 3


def stage_arms(c, fast=True):
    """(fwd, wgrad, dgrad) a ConvPoolNormFn call on a wide case reaches; fast False: SDREAMER_FAST_GEMM=0"""
    wg = _wgrad(c.nb, c.H, c.W, c.cx, c.co, c.k, fast)
    dg = "-" if not c.dx else DGRAD if fast else cm.dgrad_arm(c.H, c.W, c.co, c.cx, c.k, False)
    return _fwd(c.H, c.W, c.cx, c.co, c.k), wg, dg


def auto_slabs(nb, H, W, ci, co, k):
    """sd_conv2d_wgrad_wide3_slabs(request = 0), restated"""
    ktiles = -(-nb * H * W // BK)
    tiles = -(-co // BM) * -(-(k * k * ci + 1) // BN)
    return max(1, min(-(-1024 // tiles), ktiles // 8, 64, ktiles))


def slab_chunk(pixels, slabs):
    """pixels per slab: an equal share rounded up to the 32-pixel k tile"""
    return -(-(-(-pixels // slabs)) // BK) * BK


# ===================================================================================================== wrong references
KERNEL_MUTANTS = ("k_tail", "n_tail", "slab")


def kernel_mutant_applies(c, mut):
    N = c.ci if c.op == "dgrad" else c.k * c.k * c.ci + 1
    K = c.k * c.k * c.co if c.op == "dgrad" else c.nb * c.H * c.W
    lo = (c.k - 1) // 2  # dgrad's last k's are w's tap (0, 0): it meets the image only where H and W exceed the pad
    return {"k_tail": K % BK != 0 and (c.op == "wgrad" or (c.H > lo and c.W > lo)), "n_tail": N % BN != 0,
            "slab": c.op == "wgrad" and K > slab_chunk(K, FORCED_SLABS)}[mut]


def run_kernel_mutant(c, mut):
    """the float64 contraction with a wide-arm mistake: k_tail: the last K % 32 products dropped; n_tail: the output
    columns from 64 * (N // 64) zeroed; slab: the second of FORCED_SLABS pixel slabs skipped (bwd-weight)"""
    x, w, dout = (t.double() for t in cm.kernel_inputs(c))
    ref = cm.run_kernel_ref(c)["ref"]
    if not kernel_mutant_applies(c, mut):
        return ref.copy()
    if mut == "n_tail":
        out = ref.copy()
        N = out.shape[-1]
        out[..., BN * (N // BN):] = 0.0
        return out
    pixels = c.nb * c.H * c.W
    if c.op == "dgrad":  # k = (ky, kx, co) of the flipped weight: the last ones are tap (0, 0) of w, the last channels
        r = (c.k * c.k * c.co) % BK
        assert r < c.co
        only = torch.zeros_like(w)
        only[c.co - r:, :, 0, 0] = w[c.co - r:, :, 0, 0]
        return ref - cm._np(cm._contract(c, x, only, dout))
    keep = torch.ones(pixels, dtype=torch.bool)
    if mut == "k_tail":
        keep[pixels - pixels % BK:] = False
    else:
        ch = slab_chunk(pixels, FORCED_SLABS)
        keep[ch:2 * ch] = False
    d2 = (dout.reshape(pixels, c.co) * keep[:, None]).reshape(dout.shape)
    return cm._np(cm._contract(c, x, w, d2))


def run_stage_rms128(c):
    """the stage in float64 with the RMS sum taken over the first 128 channels only (a narrow kernel's lanes): y and the
    gradients of <y, dy>, as cm.run_stage_ref returns them (amax and conv are the reference's)"""
    x, w, b, nw, gamma, beta, dy = (None if t is None else t.clone().double() for t in cm.stage_inputs(c))
    leaves = dict(x=x, w=w, b=b, nw=nw)
    if c.ipc:
        leaves.update(gamma=gamma, beta=beta)
    for t in leaves.values():
        t.requires_grad_(True)
    conv = cm.conv_same(((x - 0.5) if c.raw else x).permute(0, 3, 1, 2), w, b)
    pooled = F.max_pool2d(conv, 2, 2).permute(0, 2, 3, 1)
    ss = (pooled[..., :WIDE_MIN] ** 2).sum(-1, keepdim=True)
    z = pooled * torch.rsqrt(ss / c.co + cm.EPS) * nw
    if c.ipc:
        rows = torch.arange(c.nb) // c.ipc
        z = gamma[rows][:, None, None, :] * z + beta[rows][:, None, None, :]
    y = F.silu(z)
    if c.nchw:
        y = y.permute(0, 3, 1, 2).reshape(c.nb, -1)
    gr = torch.autograd.grad((y * dy).sum(), list(leaves.values()))
    out = dict(cm.run_stage_ref(c), y=cm._np(y))
    for name, g in zip(leaves, gr):
        out["d" + name] = cm._np(g)
    return out


@functools.lru_cache(maxsize=None)
def conv_err(c):
    """the float32 restatement's worst conv-output error (the tie-margin rule's yardstick)"""
    return float(np.abs(cm.run_stage_ref(c, cm.F32)["conv"] - cm.run_stage_ref(c, cm.F64)["conv"]).max())


class Launches:
    """records the name of every entry point called while it is active (a _native.PROBES member that times nothing)"""

    def __init__(self):
        self.names = []

    def match(self, name, args):
        self.names.append(name)
        return False

    def __enter__(self):
        from sdreamer import _native as nat
        nat.PROBES.append(self)
        return self

    def __exit__(self, *exc):
        from sdreamer import _native as nat
        nat.PROBES.remove(self)

    def count(self, name):
        return self.names.count(name)
