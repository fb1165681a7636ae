"""Cases, guarded inputs, float64 references and comparisons for the dense contractions: csrc/gemm.hip (sd_gemm_f32)
and csrc/gemm3.hip (sd_gemm_bf16x3, _wgrad, _wgrad2, _mlp) over gemm_core.h / gemm3_core.h. Test infrastructure (a
plain module: no fixtures, no pytest hooks), in the pattern of rowop_models.py.

Shared by tests/test_gemm_parity_cpu.py (the tables reach every arm of the restated dispatch, the case conditions
hold, the two tile remaps are bijections, the float32 restatement and the split model pass their bounds with room,
planted faults fail) and tests/test_gpu_gemm_f64.py (the kernels against float64). DESIGN.md § 2.5 holds the tables
and the measured figures.

Dispatch: f32_arm / bf16x3_arm / mlp_arm / vec_ok / g3_remap / w256_remap restate the launchers' host code; each
quotes the lines it restates.

Inputs: every operand, C, the row sums, part_out and the workspace are views inside a larger allocation filled with a
NaN sentinel (Buf), at the base offset, leading dimension and batch stride the case asks for; after a launch
everything outside the view is compared bit for bit.

References: gemm_eval / mlp_eval evaluate a case as ("plain", float64) the reference, ("plain", float32) the float32
restatement, ("split", float64) the split model (hi = bf16(a), lo = bf16(a - hi), hi*hi + hi*lo + lo*hi summed in
float64: what the split-bf16 kernels compute up to their float32 accumulation), ("split", float32) the split model
accumulated in float32, each optionally with one named fault planted.

Comparison: elementwise through parity.assert_close with rtol = 0,
  f32 entries            atol_ij = k * eps32 * (|alpha| sum_k |a_ik b_kj| + |bias_j| + |beta c_ij|)
  split-bf16 vs split    atol_ij = k * eps32 * (|alpha| sum |split terms| + |bias_j| + |beta c_ij|)
  split-bf16 vs float64  atol_ij = k * (2^-17 |alpha| sum_k |a_ik b_kj| + eps32 (|bias_j| + |beta c_ij|))
  row sums               atol_i  = k * eps32 * (|alpha| sum_k |a_ik| + |rowsum_i before|)
  part_out               atol    = sum over the 64 columns of 2 |C| atol(C) + k * eps32 * sum C^2
and the existing test's figures (tests/test_gpu_gemm.py) as caps in their own form.
"""
import itertools
import zlib
from dataclasses import dataclass, replace
from types import SimpleNamespace

import numpy as np
import torch

import parity

F32, F64 = torch.float32, torch.float64
EPS32 = float(np.finfo(np.float32).eps)
U17 = 2.0 ** -17  # the split's unit: a - (hi + lo) <= 2^-17 |a|
RMS_EPS = 1e-4
GUARD = 256  # sentinel floats in front of and behind every view (a multiple of 4: the view's alignment is its own)
SD_OK, SD_EARG, SD_ESHAPE = 0, -1, -2
MAXB = 4  # SD_MLP_MAXB
SENT_BITS = 0x7FC0BEEF  # a quiet NaN with a payload: read, it poisons the output; written over, its bits change


def _g(seed):
    return torch.Generator().manual_seed(seed)


def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def cdiv(a, b):
    return -(-a // b)


def roundup(a, b):
    return cdiv(a, b) * b


# =============================================================================================== guarded buffers
class Buf:
    """A strided view inside a sentinel-filled flat float32 allocation: `front` sentinels, `off` more (the base
    offset the case asks for), the view, `back` sentinels."""

    def __init__(self, shape, strides, off=0, fill=None, front=GUARD, back=GUARD):
        self.shape, self.strides = tuple(int(s) for s in shape), tuple(int(s) for s in strides)
        ext = 0 if 0 in self.shape else 1 + sum((s - 1) * st for s, st in zip(self.shape, self.strides))
        self.start, self.ext = front + off, ext
        self.n = self.start + ext + back
        self.host = torch.full((self.n,), SENT_BITS, dtype=torch.int32).view(F32)
        if fill is not None and ext:
            fill = torch.as_tensor(fill, dtype=F32)
            lead = [i for i, st in enumerate(self.strides) if st == 0 and self.shape[i] > 1]
            if lead:  # broadcast dimension: one copy
                assert lead == [0]
                torch.as_strided(self.host, self.shape[1:], self.strides[1:], self.start).copy_(fill[0])
            else:
                self.view(self.host).copy_(fill)

    def view(self, flat):
        return torch.as_strided(flat, self.shape, self.strides, self.start)

    def inside(self):
        m = torch.zeros(self.n, dtype=torch.bool)
        if self.ext:
            m[torch.as_strided(torch.arange(self.n), self.shape, self.strides, self.start).reshape(-1)] = True
        return m

    def changed_outside(self, flat_after, also_inside=None):
        """indices outside the view (and outside `also_inside`, a bool mask of elements allowed to change) whose bits
        differ from the allocation as built"""
        a = torch.as_tensor(flat_after).cpu().view(torch.int32)
        keep = ~self.inside() if also_inside is None else ~also_inside
        return torch.nonzero((a != self.host.view(torch.int32)) & keep).reshape(-1).tolist()


def _operand(vals, kcontig, vec, bcast=False):
    """vals (batch, rows, K) -> Buf. vec: "v" vectorisable (16-B base, ld % 4 == 0, stride % 4 == 0), "pad" the same
    with ld 4 above the row, "off" base offset by one float, "ld" ld % 4 == 1, "stride" batch stride % 4 == 1."""
    Bt, R, K = vals.shape
    inner, outer = (K, R) if kcontig else (R, K)
    pad = (-inner) % 4 + {"ld": 1, "pad": 4}.get(vec, 0)
    ld = max(inner + pad, 1)
    ext = max((outer - 1) * ld + inner, 0)
    stride = 0 if bcast else roundup(ext, 4) + (1 if vec == "stride" else 0)
    strides = (stride, ld, 1) if kcontig else (stride, 1, ld)
    return Buf((Bt, R, K), strides, 1 if vec == "off" else 0, vals), ld, stride


def vec_ok(off, ld, batch, stride):
    """gemm_core.h:671-675 aligned16 / vec_ok: a 16-B aligned base, ld % 4 == 0 and a batch stride % 4 == 0"""
    return off % 4 == 0 and ld % 4 == 0 and (batch == 1 or stride % 4 == 0)


# =============================================================================================== GEMM cases
@dataclass(frozen=True)
class G:
    entry: str  # "f32" | "bf16x3" | "wgrad" | "wgrad2"
    M: int
    N: int
    K: int
    batch: int = 1
    ak: bool = True
    bk: bool = True
    va: str = "v"
    vb: str = "v"
    ksplit: int = 1
    tile: int = -1
    alpha: float = 1.0
    beta: float = 0.0
    bias: int = 1  # 0 none, 1 one row, 2 one row per batch entry (strideBias)
    padc: int = 0  # ldc - N
    bcast: bool = False  # strideA = 0
    nanc: bool = False  # C pre-filled with NaN (beta = 0)
    acc: int = 1  # wgrad: accumulate
    rs_split: int = 0  # wgrad2
    abi: bool = False  # through the C ABI (nat.call) with an explicit guarded workspace
    group: str = ""

    @property
    def name(self):
        s = (f"{self.entry}-{self.M}x{self.N}x{self.K}-b{self.batch}-{'k' if self.ak else 'm'}{'k' if self.bk else 'n'}"
             f"-{self.va}.{self.vb}-ks{self.ksplit}-t{self.tile}-a{self.alpha:g}-be{self.beta:g}-bi{self.bias}")
        s += f"-pc{self.padc}" if self.padc else ""
        s += "-bcast" if self.bcast else ""
        s += "-nanc" if self.nanc else ""
        s += f"-acc{self.acc}" if self.entry.startswith("wgrad") else ""
        s += f"-rs{self.rs_split}" if self.rs_split else ""
        s += "-abi" if self.abi else ""
        return s


@dataclass
class GemmInputs:
    A: torch.Tensor  # (batch or 1, M, K) values
    B: torch.Tensor  # (batch, N, K) values: row n, k
    bias: torch.Tensor  # (batch or 1, N) or None
    C0: torch.Tensor  # (batch, M, N)
    rs0: torch.Tensor  # (M,) the row sums' buffer before the launch
    bufA: Buf
    bufB: Buf
    bufC: Buf
    bufBias: Buf
    bufRs: Buf
    bufRs2: Buf
    bufWs: Buf
    d: SimpleNamespace  # the descriptor's numbers


def ws_floats(c):
    """sdhip.h:37,58-59: ksplit * batch * M * N slabs, + ksplit * M for the row sums' partials"""
    if c.ksplit <= 1:
        return 0
    return c.ksplit * c.batch * c.M * c.N + (c.ksplit * c.M if c.entry.startswith("wgrad") else 0)


def gemm_inputs(c):
    g = _g(seed_of(c.name))
    A = torch.randn(1 if c.bcast else c.batch, c.M, c.K, generator=g)
    B = torch.randn(c.batch, c.N, c.K, generator=g)
    bias = torch.randn(c.batch if c.bias == 2 else 1, c.N, generator=g) if c.bias else None
    C0 = torch.randn(c.batch, c.M, c.N, generator=g)
    rs0 = torch.randn(c.M, generator=g)
    bufA, lda, sA = _operand(A.expand(c.batch, c.M, c.K), c.ak, c.va, c.bcast)
    bufB, ldb, sB = _operand(B, c.bk, c.vb)
    ldc = c.N + c.padc
    sC = c.M * ldc + (8 if c.padc else 0)
    bufC = Buf((c.batch, c.M, c.N), (sC, ldc, 1), 0, torch.full_like(C0, float("nan")) if c.nanc else C0)
    sBias = roundup(c.N, 4) + 4 if c.bias == 2 else 0
    bufBias = Buf((c.batch if c.bias == 2 else 1, c.N), (sBias, 1), 0, bias) if c.bias else None
    two = c.entry == "wgrad2"
    bufRs = Buf((c.rs_split if two else c.M,), (1,), 0, rs0[:c.rs_split] if two else rs0)
    bufRs2 = Buf((c.M - c.rs_split,), (1,), 0, rs0[c.rs_split:]) if two else None
    bufWs = Buf((ws_floats(c),), (1,), 0)
    d = SimpleNamespace(M=c.M, N=c.N, K=c.K, batch=c.batch, ak=c.ak, bk=c.bk, ksplit=c.ksplit, tile=c.tile,
                        lda=lda, ldb=ldb, ldc=ldc, sA=sA, sB=sB, sC=sC, sBias=sBias, offA=bufA.start, offB=bufB.start,
                        alpha=c.alpha, beta=c.beta)
    return GemmInputs(A, B, bias, C0, rs0, bufA, bufB, bufC, bufBias, bufRs, bufRs2, bufWs, d)


# =============================================================================================== the dispatch restated
F32_TILES = {0: (128, 128), 1: (64, 64), 2: (32, 128), 3: (128, 64)}  # gemm.hip:34-39 launch_layout
G3_TILES = {0: (128, 128), 1: (64, 64), 2: (256, 128)}  # gemm3.hip:94-98 launch3_layout
G3_T128 = 192  # gemm3.hip G3_T128


def f32_arm(d):
    """gemm.hip:184-226 sd_gemm_f32 (after the null checks). Returns a refusal / no-op code or a namespace: kernel
    ("m16", "skinny", "tile0".."tile3"), AK, BKC, VA, VB (VB only with BKC in the skinny kernels), ks, kchunk, reduce,
    capped (gemm_core.h:679-684 launch_reduce: more than 4096 blocks of 256)."""
    if d.tile > 3:
        return SD_EARG
    if d.M <= 0 or d.N <= 0 or d.batch <= 0:
        return SD_OK
    ks = 1 if d.ksplit < 1 else d.ksplit
    if d.K <= 0:
        ks = 1
    skinny = d.M <= 32 and d.ak and d.tile < 0
    m16 = skinny and d.M <= 16
    kgran = 16 if m16 else 32 if skinny else 32
    kc = roundup(cdiv(d.K if d.K > 0 else 1, ks), kgran)
    va, vb = vec_ok(d.offA, d.lda, d.batch, d.sA), vec_ok(d.offB, d.ldb, d.batch, d.sB)
    if skinny:
        return SimpleNamespace(kernel="m16" if m16 else "skinny", AK=True, BKC=d.bk, VA=va, VB=d.bk and vb, ks=ks,
                               kchunk=kc, reduce=ks > 1, capped=False, order="plain", RS=False)
    tile = d.tile
    if tile < 0:
        tiles128 = cdiv(d.M, 128) * cdiv(d.N, 128) * d.batch * ks
        tile = 2 if d.M <= 32 else 0 if tiles128 >= 256 else 1
    return SimpleNamespace(kernel=f"tile{tile}", AK=d.ak, BKC=d.bk, VA=va, VB=vb, ks=ks, kchunk=kc, reduce=ks > 1,
                           capped=ks > 1 and cdiv(d.batch * d.M * d.N, 256) > 4096, order="plain", RS=False)


def bf16x3_arm(d, rowsum=False, rs_split=None):
    """gemm3.hip:462-526 sd_gemm_bf16x3 / _wgrad / _wgrad2 and gemm3_run. kernel "g3tile0/1/2", or the f32 arm when
    M, N or K < 64 (sd_gemm_bf16x3 only), asked (the tile asked for, to show tile 2's downgrade), RS (the fused row
    sums), order ("plain" or "bcastA": g3_tile's batch-inside-rows order)."""
    if d.tile > 3:
        return SD_EARG
    if d.M <= 0 or d.N <= 0 or (not rowsum and d.batch <= 0):
        return SD_OK
    small = d.M < 64 or d.N < 64 or d.K < 64
    if rowsum:
        if small or d.batch != 1 or d.ak:
            return SD_ESHAPE
        if rs_split is not None and (rs_split <= 0 or rs_split >= d.M):
            return SD_ESHAPE
    elif small:
        a = f32_arm(d)
        if not isinstance(a, int):
            a.fallback = True
        return a
    ks = 1 if d.ksplit < 1 else d.ksplit
    kc = roundup(cdiv(d.K, ks), 32)
    tile = d.tile
    if tile not in (0, 1, 2):
        tiles128 = cdiv(d.M, 128) * cdiv(d.N, 128) * d.batch * ks
        tile = 0 if tiles128 >= G3_T128 else 1
    asked = tile
    if tile == 2 and (d.ak or d.bk):
        tile = 0
    bm, bn = G3_TILES[tile]
    return SimpleNamespace(kernel=f"g3tile{tile}", asked=asked, AK=d.ak, BKC=d.bk,
                           VA=vec_ok(d.offA, d.lda, d.batch, d.sA), VB=vec_ok(d.offB, d.ldb, d.batch, d.sB), ks=ks,
                           kchunk=kc, reduce=ks > 1, capped=ks > 1 and cdiv(d.batch * d.M * d.N, 256) > 4096,
                           RS=bool(rowsum) and not d.ak,
                           order="bcastA" if d.sA == 0 and d.batch > 1 and ks == 1 else "plain",
                           grid=(cdiv(d.N, bn), cdiv(d.M, bm), d.batch * ks))


def arm_of(c, d):
    if c.entry == "f32":
        return f32_arm(d)
    return bf16x3_arm(d, c.entry.startswith("wgrad"), c.rs_split if c.entry == "wgrad2" else None)


def g3_remap(L, nx, ny, nz, bcast, fault=None):
    """gemm3.hip:24-38 g3_tile: linear workgroup id -> (tx, ty, tz)"""
    T = nx * ny * nz
    per, rem, xcd, slot = T // 8, T % 8, L % 8, L // 8
    if fault == "remap_rem":
        rem = (T + 1) % 8
    L = xcd * per + (xcd if xcd < rem else rem) + slot
    if bcast:
        return L % nx, L // (nx * nz), (L // nx) % nz
    return L % nx, (L // nx) % ny, L // (nx * ny)


def w256_remap(L, T, batch, fault=None):
    """gemm3.hip:277-280 gemm3_w256_kernel: linear workgroup id -> (batch entry, row tile)"""
    per, rem, xcd, slot = T // 8, T % 8, L % 8, L // 8
    if fault == "remap_rem":
        rem = (T + 1) % 8
    L = xcd * per + (xcd if xcd < rem else rem) + slot
    return L % batch, L // batch


def is_bijection(cells, expect):
    return sorted(cells) == sorted(expect)


# =============================================================================================== GEMM evaluation
GEMM_FAULTS = ("drop_last_k", "split_no_granule", "bias_per_split", "beta_twice", "tail_quad_swap")
SPLIT_FAULTS = ("drop_hi_lo", "lo_from_a")
RS_FAULTS = ("rowsum_first_split", "rowsum_no_alpha", "rs_split_tile")
MLP_FAULTS = ("pout_tile_cols", "rstd_part0", "wrows_bias")


def bf16_split(a, fault=None):
    hi = a.to(torch.bfloat16).to(F32)
    lo = (a if fault == "lo_from_a" else a - hi).to(torch.bfloat16).to(F32)
    return hi, lo


def _products(a, b, kind, dt, fault=None):
    """a (.., M, k), b (.., N, k) float32 -> (a . b^T, sum |terms|) in dt"""
    if kind == "plain":
        x, y = a.to(dt), b.to(dt)
        return x @ y.transpose(-1, -2), x.abs() @ y.abs().transpose(-1, -2)
    (ah, al), (bh, bl) = bf16_split(a, fault), bf16_split(b, fault)
    ah, al, bh, bl = (t.to(dt) for t in (ah, al, bh, bl))
    T = lambda t: t.transpose(-1, -2)  # noqa: E731
    v = al @ T(bh) + ah @ T(bh)
    s = al.abs() @ T(bh.abs()) + ah.abs() @ T(bh.abs())
    if fault != "drop_hi_lo":
        v = v + ah @ T(bl)
        s = s + ah.abs() @ T(bl.abs())
    return v, s


def _tail_swap(X):
    """the t = rows % 4 tail rows of a rows-contiguous operand against its first t k's: the t x t block transposed"""
    R, K = X.shape[-2:]
    t = R % 4
    if t < 2 or K < t:
        return X
    X = X.clone()
    X[..., R - t:, :t] = X[..., R - t:, :t].transpose(-1, -2).clone()
    return X


def gemm_eval(c, inp, kind="plain", dt=F64, fault=None):
    """{"C", "C@scale" (the atol's sum: |alpha| sum |terms| + |bias| + |beta c|), "C@ab" (|alpha| sum |a||b|),
    "C@add" (|bias| + |beta c|), "rowsum", "rowsum@scale"[, "rowsum2", "rowsum2@scale"]} as float64 ndarrays"""
    arm = arm_of(c, inp.d)
    A, B = inp.A.expand(c.batch, c.M, c.K), inp.B
    if fault == "drop_last_k" and c.K % 4:
        A = A.clone()
        A[..., c.K - 1] = 0
    if fault == "tail_quad_swap":
        if not c.ak:
            A = _tail_swap(A)
        elif not c.bk:
            B = _tail_swap(B)
    ks, kc = arm.ks, arm.kchunk
    step = cdiv(max(c.K, 1), ks) if fault == "split_no_granule" else kc
    acc = torch.zeros(c.batch, c.M, c.N, dtype=dt)
    scale = torch.zeros(c.batch, c.M, c.N, dtype=F64)
    alpha = torch.tensor(c.alpha, dtype=dt)
    for s in range(ks):
        k0, k1 = s * step, min(c.K, s * step + kc)
        if k1 <= k0:
            continue
        v, sc = _products(A[..., k0:k1], B[..., k0:k1], kind, dt, fault)
        acc = acc + alpha * v
        scale = scale + abs(c.alpha) * sc.to(F64)
    ab = abs(c.alpha) * (A.to(F64).abs() @ B.to(F64).abs().transpose(-1, -2))
    add = torch.zeros_like(scale)
    out = acc
    if c.bias:
        bv = inp.bias.to(dt)[:, None, :]
        out = out + bv * (ks if fault == "bias_per_split" and ks > 1 else 1)
        add = add + inp.bias.to(F64).abs()[:, None, :]
    if c.beta != 0:
        bc = torch.tensor(c.beta, dtype=dt) * inp.C0.to(dt)
        out = out + bc * (2 if fault == "beta_twice" and ks > 1 else 1)
        add = add + bc.to(F64).abs()
    r = {"C": out, "C@scale": scale + add, "C@ab": ab, "C@add": add}
    if c.entry.startswith("wgrad"):
        kk = min(c.K, kc) if fault == "rowsum_first_split" and ks > 1 else c.K
        a0 = A[0, :, :kk].to(dt)
        rs = (1.0 if fault == "rowsum_no_alpha" else alpha) * a0.sum(-1)
        sc = abs(c.alpha) * A[0].to(F64).abs().sum(-1)
        keep = inp.rs0.to(dt)
        full = sc + (inp.rs0.to(F64).abs() if c.acc else 0)
        if c.entry == "wgrad2":
            cut = (c.rs_split // 64) * 64 if fault == "rs_split_tile" else c.rs_split
            b1, b2 = keep[:c.rs_split], keep[c.rs_split:]
            o1, o2 = b1.clone(), b2.clone()  # rows a (faulty) launch does not reach keep the buffer's values
            for m in range(c.M):
                tgt, src, i = (o1, b1, m) if m < cut else (o2, b2, m - cut)
                if i < len(tgt):
                    tgt[i] = (src[i] if c.acc else 0) + rs[m]
            r["rowsum"], r["rowsum2"] = o1, o2
            r["rowsum@scale"], r["rowsum2@scale"] = full[:c.rs_split], full[c.rs_split:]
        else:
            r["rowsum"] = (keep if c.acc else 0) + rs
            r["rowsum@scale"] = full
    return {k: v.to(F64).numpy() for k, v in r.items()}


# =============================================================================================== MLP cases
@dataclass(frozen=True)
class Mlp:
    M: int
    N: int
    K: int
    batch: int = 1
    rms: bool = False
    pout: bool = False
    npin: int = 1
    act: int = 1
    rows: tuple = ()  # per-entry form: entry b's weight rows (w_rows); () = the strided batch
    null: int = -1  # per-entry form through the C ABI: this entry's pointers null (the strided operand serves it)
    bcast: bool = False
    alpha: float = 1.0
    group: str = ""

    @property
    def name(self):
        s = f"mlp-{self.M}x{self.N}x{self.K}-b{self.batch}-rms{int(self.rms)}-po{int(self.pout)}"
        s += f"-q{self.npin}-act{self.act}" if self.rms else ""
        s += ("-rows" + ".".join(map(str, self.rows))) if self.rows else ""
        s += f"-null{self.null}" if self.null >= 0 else ""
        s += "-bcast" if self.bcast else ""
        s += f"-a{self.alpha:g}" if self.alpha != 1 else ""
        return s


def mlp_desc(c, **over):
    """the numbers sd_gemm_bf16x3_mlp's checks read, for a case as tests/test_gpu_gemm_f64.py launches it"""
    lda = roundup(c.K, 4)
    d = dict(M=c.M, N=c.N, K=c.K, batch=c.batch, ak=True, bk=True, beta=0.0, lda=lda, ldb=c.K, offA=0, offB=0,
             sA=0 if c.bcast else roundup(c.M * lda, 4), sB=0 if c.rows else c.N * c.K, norm_w=c.rms and (not c.rows or c.null >= 0),
             norm_w_ptr=tuple(c.rms and bool(c.rows) and b != c.null for b in range(min(c.batch, MAXB))),
             norm_w_aligned=True, stride_norm_w=c.K, part_in=c.rms, npart_in=c.npin if c.rms else 0,
             part_out=c.pout, stride_part_out=(c.N // 64) * c.M,
             w_rows=tuple((r if r < c.N else 0) for r in c.rows) if c.rows else (), w_ptr_aligned=True,
             per_entry=bool(c.rows), x=True)
    d.update(over)
    return SimpleNamespace(**d)


def mlp_arm(d, env_now256=False):
    """gemm3.hip:407-455 sd_gemm_bf16x3_mlp (after the null checks of d, A, B, C): a refusal code, SD_OK for an
    empty problem, or (kernel, RMS, POUT) with kernel "w256" (gemm3_w256_kernel) or "mlp128" (gemm3_mlp_kernel)"""
    if not d.x:
        return SD_EARG
    if d.M <= 0 or d.N <= 0 or d.batch <= 0:
        return SD_OK
    if not d.ak or not d.bk or d.K % 32 or d.K < 32 or d.N < 64 or d.beta != 0:
        return SD_ESHAPE
    if not vec_ok(d.offA, d.lda, d.batch, d.sA) or not vec_ok(d.offB, d.ldb, d.batch, d.sB):
        return SD_ESHAPE
    rms = bool(d.norm_w) or any(d.norm_w_ptr)
    if rms and (not d.part_in or d.npart_in <= 0 or (d.norm_w and (not d.norm_w_aligned or d.stride_norm_w % 4))):
        return SD_EARG
    if rms and not d.norm_w:
        for b in range(d.batch):
            if b >= MAXB or not d.norm_w_ptr[b]:
                return SD_EARG
    if d.part_out and d.N % 64:
        return SD_ESHAPE
    if d.part_out and d.batch > 1 and d.stride_part_out < (d.N // 64) * d.M:
        return SD_EARG
    for r in d.w_rows:
        if r < 0 or r > d.N:
            return SD_EARG
    if not d.w_ptr_aligned:
        return SD_ESHAPE
    if d.per_entry and d.batch > MAXB:
        return SD_EARG
    if not rms and d.N == 256 and cdiv(d.M, 256) * d.batch >= 192 and not env_now256:
        return ("w256", False, bool(d.part_out))
    return ("mlp128", rms, bool(d.part_out))


@dataclass
class MlpInputs:
    x: torch.Tensor  # (batch or 1, M, K)
    W: list  # per entry (rows_b, K)
    bias: list  # per entry (rows_b,)
    nw: torch.Tensor  # (batch, K)
    pin: torch.Tensor  # (batch, npin, M)
    bufX: Buf
    bufC: Buf
    bufPin: Buf
    bufPout: Buf
    bufW: list  # per-entry form: one Buf per entry; strided: [one Buf (batch, N, K)]
    bufBias: list
    bufNw: list


def mlp_rows(c):
    return [(c.rows[b] if c.rows else c.N) for b in range(c.batch)]


def mlp_inputs(c):
    g = _g(seed_of(c.name))
    nx = 1 if c.bcast else c.batch
    x = torch.randn(nx, c.M, c.K, generator=g) * 2
    rows = mlp_rows(c)
    W = [torch.randn(r, c.K, generator=g) / c.K ** 0.5 for r in rows]
    bias = [torch.randn(r, generator=g) * 0.3 for r in rows]
    nw = 1 + 0.1 * torch.randn(c.batch, c.K, generator=g)
    # the producer's partials: the row's sum of squares cut into npin unequal float32 parts
    ssq = (x.expand(c.batch, c.M, c.K) ** 2).sum(-1)
    cut = torch.rand(c.batch, c.npin, c.M, generator=g) + 0.1
    pin = (cut / cut.sum(1, keepdim=True) * ssq[:, None]).to(F32)
    bufX, _, _ = _operand(x.expand(c.batch, c.M, c.K), True, "v", c.bcast)
    bufC = Buf((c.batch, c.M, c.N), (c.M * c.N, c.N, 1), 0, torch.full((c.batch, c.M, c.N), float("nan")))
    bufPin = Buf((c.batch, c.npin, c.M), (c.npin * c.M, c.M, 1), 0, pin)
    nq = c.N // 64
    # behind part_out: at least one whole extra partial (M floats), so that an overrun by one partial is seen, not a fault
    bufPout = Buf((c.batch, nq, c.M), (nq * c.M, c.M, 1), 0, back=GUARD + roundup(c.M, 4)) if c.pout else None
    if c.rows:
        bufW = [Buf(w.shape, (c.K, 1), 0, w) for w in W]
        bufBias = [Buf(b.shape, (1,), 0, b) for b in bias]
        bufNw = [Buf((c.K,), (1,), 0, nw[b]) for b in range(c.batch)]
    else:
        bufW = [Buf((c.batch, c.N, c.K), (c.N * c.K, c.K, 1), 0, torch.stack(W))]
        bufBias = [Buf((c.batch, c.N), (c.N, 1), 0, torch.stack(bias))]
        bufNw = [Buf((c.batch, c.K), (c.K, 1), 0, nw)]
    return MlpInputs(x, W, bias, nw, pin, bufX, bufC, bufPin, bufPout, bufW, bufBias, bufNw)


def mlp_A(c, inp, dt, fault=None):
    """the A operand act(x * rstd * nw), rstd = 1 / sqrt(sum_q part_in / K + eps) (gemm3.hip:187-196, KC3Rms::store)"""
    x = inp.x.expand(c.batch, c.M, c.K).to(dt)
    if not c.rms:
        return x
    pin = inp.pin.to(dt)
    s = pin[:, 0] if fault == "rstd_part0" else pin.sum(1) if dt == F64 else sum(pin[:, q] for q in range(c.npin))
    rstd = 1 / torch.sqrt(s / c.K + torch.tensor(RMS_EPS, dtype=F32).to(dt))
    y = x * rstd[:, :, None] * inp.nw.to(dt)[:, None, :]
    return y * torch.sigmoid(y) if c.act else y


def mlp_eval(c, inp, kind="plain", dt=F64, fault=None):
    """{"C", "C@scale", "C@ab", "C@add", "pout", "pout@sq"}: the split kinds form A in float32 as the kernel does and
    split that; the plain kinds form it in dt"""
    A = mlp_A(c, inp, F32 if kind == "split" else dt, fault)
    rows = mlp_rows(c)
    C = torch.zeros(c.batch, c.M, c.N, dtype=dt)
    scale = torch.zeros(c.batch, c.M, c.N, dtype=F64)
    ab, add = torch.zeros_like(scale), torch.zeros_like(scale)
    for b in range(c.batch):
        r = rows[b]
        v, sc = _products(A[b].to(F32) if kind == "split" else A[b], inp.W[b], kind, dt, fault)
        C[b, :, :r] = torch.tensor(c.alpha, dtype=dt) * v + inp.bias[b].to(dt)
        scale[b, :, :r] = abs(c.alpha) * sc.to(F64) + inp.bias[b].to(F64).abs()
        ab[b, :, :r] = abs(c.alpha) * (A[b].to(F64).abs() @ inp.W[b].to(F64).abs().t())
        add[b, :, :r] = inp.bias[b].to(F64).abs()
        if fault == "wrows_bias" and r < c.N:  # a bias value where the columns past the entry's rows hold 0
            C[b, :, r:] = 0.25
    out = {"C": C, "C@scale": scale, "C@ab": ab, "C@add": add}
    if c.rms and kind == "split":
        # The model forms A = act(x rstd nw) in float32 and so does the kernel, with other roundings (v_rsq_f32, its
        # own exp and reciprocal): two float32 evaluations of a differ by up to d = u eps32 |a|, u <= 2 (2.5 (rstd and
        # the two products) + 3 (the sigmoid) + 2.5 (1 + |y|) (the sigmoid's argument, |y| <= 6)) < 64, and where a
        # moves, lo = bf16(a - hi) may round the other way: hi + lo moves by up to d + 2^-17 |a|. So against the split
        # model an entry with an input norm is held to the float32 sum's bound plus 2 * 2^-17 |alpha| sum |a||b|.
        out["C@form"] = 2 * U17 * ab
    if c.pout:
        sq = (C * C).reshape(c.batch, c.M, c.N // 64, 64).sum(-1).transpose(1, 2)  # (batch, N / 64, M)
        if fault == "pout_tile_cols":
            q = torch.arange(c.N // 64) % 2
            sq = sq[:, q]
        out["pout"], out["pout@sq"] = sq, sq.to(F64)
    return {k: v.to(F64).numpy() for k, v in out.items()}


# =============================================================================================== tolerances
@dataclass(frozen=True)
class Tol:
    k: float  # the multiple of the output's own unit
    cap: float  # the existing test's figure, in the same unit where the forms agree (else asserted in its own form)


CAP_F32 = 2e-6 / EPS32  # tests/test_gpu_gemm.py: 2e-6 * sum|a||b|  = 16.8 float32 epsilons
CAP_G3 = 4e-5 / U17  # 4e-5 * sum|a||b| = 5.24 units of 2^-17
CAP_REL = 1e-5 / EPS32  # 1e-5 relative for the row sums and partials = 83.9 float32 epsilons
# Each k is 8 x the larger of two measured distances from float64 in the output's own unit, the CPU column's and the
# MI355X's (DESIGN.md § 2.5 lists both per output), worst over the family's cases; where that exceeds the cap, the cap.
TOL = {
    "f32": {"C": Tol(CAP_F32, CAP_F32)},  # 8 x 3.24 is above the cap
    "bf16x3": {"C_split": Tol(15.7, CAP_F32), "C": Tol(CAP_G3, CAP_G3)},  # C: 8 x 0.70 is above the cap
    "wgrad": {"C_split": Tol(11.0, CAP_F32), "C": Tol(CAP_G3, CAP_G3), "rowsum": Tol(4.5, CAP_REL)},
    # part_out: both columns measured 0 beyond C's carried bound; the float32 sum of 64 squares over a shuffle tree, one
    # rounding per product and per level, stays below 2 eps32 sum C^2
    "mlp": {"C_split": Tol(15.9, CAP_F32), "C": Tol(CAP_G3, CAP_G3), "pout": Tol(2.0, CAP_REL)},  # C: 8 x 1.46
}
for _f in TOL.values():
    assert all(t.k <= t.cap for t in _f.values())


def family(c):
    if isinstance(c, Mlp):
        return "mlp"
    return "wgrad" if c.entry.startswith("wgrad") else c.entry


def routed_f32(c, arm):
    """a split-bf16 entry's case that the f32 kernels serve (M, N or K < 64): held to the f32 tolerance"""
    return getattr(arm, "fallback", False)


def atols(fam, ref, split, k=None, only=None):
    """{comparison: (reference array, atol array)} at the family's tolerances; k, only: comparison `only` at k units"""
    kk = lambda name: k if name == only else TOL[fam][name].k  # noqa: E731
    out = {}
    if fam == "f32":
        out["C"] = (ref["C"], kk("C") * EPS32 * ref["C@scale"])
    else:
        # "C@form" (the MLP entry's input norm): what forming A in float32 twice may differ by, see mlp_eval
        out["C_split"] = (split["C"], kk("C_split") * EPS32 * split["C@scale"] + split.get("C@form", 0.0))
        out["C"] = (ref["C"], kk("C") * (U17 * ref["C@ab"] + EPS32 * ref["C@add"]))
    for rs in ("rowsum", "rowsum2"):
        if rs in ref:
            out[rs] = (ref[rs], (k if only in ("rowsum", "rowsum2") else TOL[fam]["rowsum"].k) * EPS32 * ref[rs + "@scale"])
    if "pout" in ref:
        # C's own bound carried into the sum of squares, + the float32 sum of the 64 squares
        catol = out["C"][1]
        B_, M_, N_ = ref["C"].shape
        carried = (2 * np.abs(ref["C"]) * catol).reshape(B_, M_, N_ // 64, 64).sum(-1).transpose(0, 2, 1)
        out["pout"] = (ref["pout"], carried + kk("pout") * EPS32 * ref["pout@sq"])
    return out


def units(fam, got, ref, split):
    """{comparison: max error in the comparison's own unit}: what k would have to be for the element furthest out
    (the parts of a bound that do not scale with k, the A-forming allowance and part_out's carried bound, taken off)"""
    res = {}
    for name in atols(fam, ref, split):
        r, a0 = atols(fam, ref, split, 0.0, name)[name]
        a1 = atols(fam, ref, split, 1.0, name)[name][1]
        g = got["C"] if name == "C_split" else got[name]
        if r.size == 0:
            continue
        e = np.maximum(np.abs(g - r) - a0, 0) / np.maximum(a1 - a0, 1e-300)
        res[name] = float(np.where(a1 - a0 > 0, e, 0.0).max())
    return res


def caps_ok(fam, got, ref):
    """the existing tests' bounds in their own form (tests/test_gpu_gemm.py), per output: [] or what failed"""
    bad = []
    err = np.abs(got["C"] - ref["C"])
    if fam == "f32":
        if err.size and err.max() > 2e-6 * (ref["C@ab"].max() + 1):
            bad.append("C above 2e-6 * (max sum|a||b| + 1)")
    elif err.size and (err > 4e-5 * ref["C@ab"] + 1e-5 * (1 + ref["C@add"])).any():
        bad.append("C above 4e-5 * sum|a||b| + 1e-5 (1 + |c| + |bias|)")
    for rs in ("rowsum", "rowsum2"):
        if rs in ref and ref[rs].size:
            e = np.abs(got[rs] - ref[rs])
            if (e > 1e-5 * np.abs(ref[rs]) + 1e-6 * ref[rs + "@scale"].max()).any():
                bad.append(f"{rs} above 1e-5 relative + 1e-6 max sum|a|")
    if "pout" in ref and "pout_own" in got:  # against the launch's own C, as the existing test does
        if (np.abs(got["pout"] - got["pout_own"]) > 1e-5 * got["pout_own"] + 1e-6).any():
            bad.append("pout above 1e-5 relative + 1e-6 of its own C's squares")
    return bad


def failures(fam, got, ref, split, arm=None):
    """[] or the list of comparisons `got` fails (elementwise bounds, finiteness, the caps)"""
    if routed_f32(None, arm):
        fam_c = "f32"
    else:
        fam_c = fam
    bad = []
    for name, (r, a) in atols(fam_c, ref, split).items():
        g = got["C"] if name == "C_split" else got[name]
        if g.shape != r.shape:
            bad.append(f"{name}: shape {g.shape} vs {r.shape}")
            continue
        if not np.isfinite(g).all():
            bad.append(f"{name}: not finite")
            continue
        try:
            parity.assert_close(g, r, 0.0, a, name)
        except AssertionError as e:
            bad.append(str(e))
    return bad + caps_ok(fam_c, got, ref)


def own_pout(C):
    B_, M_, N_ = C.shape
    return (np.asarray(C, np.float64) ** 2).reshape(B_, M_, N_ // 64, 64).sum(-1).transpose(0, 2, 1)


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a if "@" not in k)


# =============================================================================================== the case tables
def _cyc(seq, i):
    return seq[i % len(seq)]


def _skinny_cases(kind):
    Ms, Ns, Ks = ((1, 16), (1, 15, 17), (1, 15, 512, 513, 1100)) if kind == "m16" else \
        ((17, 32), (1, 31, 33), (1, 31, 128, 129, 300))
    out, seen = [], {True: 0, False: 0}
    for i, (M, N, K, bk) in enumerate(itertools.product(Ms, Ns, Ks, (True, False))):
        # every (VA, VB, reduce) of this B layout in turn (a B with n contiguous has no vector form)
        combos = list(itertools.product((True, False), (True, False) if bk else (True,), (False, True)))
        va_on, vb_on, red = combos[seen[bk] % len(combos)]
        seen[bk] += 1
        batch = 3 if i % 4 == 1 else 1
        va = _cyc(("v", "pad"), i) if va_on else _cyc(("off", "ld", "stride" if batch > 1 else "ld"), i // 2)
        vb = _cyc(("pad", "v"), i) if vb_on else _cyc(("ld", "off"), i // 2)
        out.append(G("f32", M, N, K, batch=batch, bk=bk, va=va, vb=vb, ksplit=3 if red else 1,
                     bias=2 if batch > 1 else _cyc((1, 0), i // 3), beta=_cyc((0.0, 1.0), i // 5), group=kind))
    M = Ms[1]
    out += [G("f32", M, Ns[2], 40, ksplit=4, group=kind),  # chunk 16 / 32: the last split(s) empty
            G("f32", M, Ns[1], 40, ksplit=4, bk=False, batch=3, bias=2, beta=1.0, alpha=0.5, padc=3, group=kind),
            G("f32", M, Ns[2], Ks[4], nanc=True, group=kind), G("f32", M, Ns[2], Ks[4], nanc=True, ksplit=3, group=kind)]
    return out


def _tile_cases():
    out = []
    for i, (tile, ak, bk, va_on, vb_on, red) in enumerate(itertools.product((0, 1, 2, 3), *[(True, False)] * 5)):
        bm, bn = F32_TILES[tile]
        K = _cyc((37, 64), i // 2 + i // 8 + tile)  # ragged in both dimensions, a second tile in each; K % 4 != 0 at 37
        va = "v" if va_on else _cyc(("ld", "off"), i // 4)
        vb = "pad" if vb_on else _cyc(("off", "ld"), i // 4)
        out.append(G("f32", bm + 2, bn + 5, K, ak=ak, bk=bk, va=va, vb=vb, ksplit=3 if red else 1, tile=tile,
                     beta=_cyc((0.0, 1.0), i), bias=_cyc((1, 1, 0), i), group="tiles"))
    return out


F32_EXTRA = [
    G("f32", 33, 1, 1, batch=256, bias=2, group="auto"),  # 256 tiles of 128 -> tile 0
    G("f32", 33, 1, 1, group="auto"),  # -> tile 1
    G("f32", 20, 40, 50, ak=False, group="auto"),  # M <= 32 off the skinny kernels -> tile 2
    G("f32", 33, 64, 64, batch=497, ksplit=2, bias=2, group="capped"),  # 4101 reduce blocks, capped at 4096
    G("f32", 5, 7, 0, beta=1.0, abi=True, group="k0"), G("f32", 40, 9, 0, ksplit=3, batch=2, bias=2, abi=True, group="k0"),
    G("f32", 20, 9, 0, ak=False, beta=0.5, bias=0, abi=True, group="k0"),
    G("f32", 66, 69, 37, tile=1, nanc=True, group="edge"), G("f32", 66, 69, 37, tile=1, nanc=True, ksplit=3, group="edge"),
    G("f32", 66, 69, 37, tile=1, alpha=0.5, beta=1.0, padc=3, group="edge"),
    G("f32", 66, 69, 37, tile=1, alpha=0.5, beta=1.0, padc=3, ksplit=3, batch=2, bias=2, group="edge"),
    G("f32", 66, 69, 64, tile=0, ksplit=2, abi=True, group="edge"),  # the workspace at exactly its contract size
    G("f32", 16, 17, 513, ksplit=3, abi=True, group="edge"), G("f32", 32, 33, 300, ksplit=3, abi=True, group="edge"),
]
F32_CASES = _skinny_cases("m16") + _skinny_cases("skinny") + _tile_cases() + F32_EXTRA


def _g3_cases():
    out = [G("bf16x3", 63, 64, 64, abi=True, group="fallback"), G("bf16x3", 64, 63, 64, abi=True, group="fallback"),
           G("bf16x3", 64, 64, 63, abi=True, group="fallback"),
           G("bf16x3", 130, 65, 96, tile=1, group="g3"), G("bf16x3", 130, 130, 96, tile=0, group="g3"),
           G("bf16x3", 64, 64, 64, batch=192, bias=2, group="g3"),  # 192 tiles of 128 -> tile 0
           G("bf16x3", 257, 130, 96, ak=False, bk=False, tile=2, group="g3"),
           G("bf16x3", 257, 130, 96, ak=False, bk=False, tile=2, ksplit=3, beta=1.0, abi=True, group="g3"),
           G("bf16x3", 257, 130, 96, ak=True, bk=False, tile=2, group="g3"),  # tile 2 asked, runs tile 0
           G("bf16x3", 130, 65, 71, ak=False, bk=True, tile=2, group="g3"),
           G("bf16x3", 64, 64, 64, ksplit=3, group="g3"),  # chunk 32: the third split empty
           G("bf16x3", 65, 130, 64, ksplit=3, ak=False, bk=False, beta=1.0, alpha=0.5, padc=5, group="g3"),
           G("bf16x3", 65, 130, 96, nanc=True, group="g3"), G("bf16x3", 65, 130, 96, nanc=True, ksplit=3, group="g3"),
           # A broadcast over the batch: ksplit 1 takes the batch-inside-rows order, ksplit 2 the plain one
           G("bf16x3", 130, 65, 96, batch=4, bcast=True, bias=2, tile=1, group="bcast"),
           G("bf16x3", 130, 65, 96, batch=4, bcast=True, bias=2, tile=1, ksplit=2, group="bcast"),
           G("bf16x3", 64, 65, 64, batch=2, bcast=True, tile=1, group="bcast"),  # 4 tiles (< 8)
           G("bf16x3", 130, 65, 71, batch=3, bcast=True, bias=2, tile=1, ak=False, group="bcast"),  # 18 tiles
           G("bf16x3", 130, 130, 64, batch=3, bcast=True, tile=0, group="bcast"),  # 3 tiles of 128... per entry 2 x 2
           # tile counts 3, 8, 15, 193
           G("bf16x3", 64, 192, 64, tile=1, group="count"), G("bf16x3", 128, 256, 64, tile=1, group="count"),
           G("bf16x3", 192, 320, 64, tile=1, group="count"), G("bf16x3", 64, 64, 64, batch=193, tile=1, group="count"),
           # the unvectorised loaders from a misaligned base and from a batch stride off a multiple of 4
           G("bf16x3", 65, 64, 71, batch=2, va="stride", vb="stride", bias=2, tile=1, group="g3"),
           G("bf16x3", 65, 64, 71, batch=2, va="stride", vb="stride", ak=False, bk=False, tile=0, group="g3")]
    shapes = [(M, N, _cyc((64, 71, 96), i)) for i, (M, N) in enumerate(itertools.product((64, 65, 130), (64, 65, 130)))]
    for i, ((si, (M, N, K)), ak, bk, va_on, vb_on) in enumerate(itertools.product(enumerate(shapes),
                                                                                 *[(True, False)] * 4)):
        va = _cyc(("v", "pad"), i) if va_on else _cyc(("off", "ld"), si)
        vb = _cyc(("pad", "v"), i) if vb_on else _cyc(("ld", "off"), si)
        out.append(G("bf16x3", M, N, K, ak=ak, bk=bk, va=va, vb=vb, ksplit=_cyc((1, 3), i // 16 + i),
                     tile=_cyc((0, 1), si + i), beta=_cyc((0.0, 1.0), i // 5), alpha=_cyc((1.0, 0.5), i // 7),
                     bias=_cyc((1, 0), i // 4), group="layouts"))
    return out


def _wgrad_cases():
    shapes = list(itertools.product((64, 65, 257), (64, 130), (64, 96, 100)))
    out = []
    for i, (tile, bk, ks, acc, alpha) in enumerate(itertools.product((0, 1, 2), (True, False), (1, 3), (0, 1),
                                                                   (1.0, 0.5))):
        M, N, K = _cyc(shapes, 5 * i + 1)
        out.append(G("wgrad", M, N, K, ak=False, bk=bk, ksplit=ks, tile=tile, acc=acc, alpha=alpha, beta=1.0, bias=0,
                     va=_cyc(("v", "ld", "pad"), i), vb=_cyc(("v", "off"), i // 2), abi=(acc == 0 or ks > 1),
                     group="wgrad"))
    for i, rs in enumerate((1, 64, 65, 256)):  # 256 = M - 1
        for ks in (1, 3):
            out.append(G("wgrad2", 257, 130, _cyc((64, 96, 100), i), ak=False, bk=False, ksplit=ks,
                         tile=_cyc((2, 0, 1), i + ks), acc=_cyc((1, 0), i + ks // 2), alpha=_cyc((1.0, 0.5), i),
                         beta=1.0, bias=0, rs_split=rs, abi=True, group="wgrad2"))
    out += [G("wgrad2", 65, 64, 100, ak=False, bk=True, rs_split=64, beta=1.0, bias=0, abi=True, group="wgrad2"),
            G("wgrad", 64, 64, 64, ak=False, bk=False, ksplit=3, beta=1.0, bias=0, abi=True, group="wgrad"),
            # through kernels.wgrad / kernels.wgrad2 (their own split choice)
            G("wgrad", 130, 64, 1100, ak=False, bk=False, ksplit=2, beta=1.0, bias=0, group="wgrad-py"),
            G("wgrad2", 130, 64, 1100, ak=False, bk=False, ksplit=2, beta=1.0, bias=0, rs_split=65, group="wgrad-py")]
    return out


G3_CASES = _g3_cases()
WGRAD_CASES = _wgrad_cases()


def _mlp_cases():
    out = []
    for i, (N, M) in enumerate(itertools.product((64, 128, 192, 256, 320), (1, 127, 129))):
        for rms in (False, True):
            out.append(Mlp(M, N, _cyc((32, 96), i), batch=_cyc((1, 3, 5), i + rms), rms=rms, pout=True,
                           npin=_cyc((1, 3), i), act=_cyc((1, 0), i // 2), group="pout"))
    for i, (N, M, rms) in enumerate(itertools.product((65, 255), (1, 127, 129), (False, True))):
        out.append(Mlp(M, N, _cyc((96, 32), i), batch=_cyc((3, 1, 5), i), rms=rms, npin=_cyc((3, 1), i),
                       act=_cyc((0, 1), i // 2), alpha=_cyc((1.0, 0.5), i // 3), group="nopout"))
    # N = 64 * odd with part_out, batch > 1, strided and per entry (the last tile's second half lies past N)
    for N in (64, 192, 320):
        out += [Mlp(129, N, 32, batch=3, rms=False, pout=True, group="odd"),
                Mlp(129, N, 32, batch=3, rms=True, pout=True, npin=3, group="odd"),
                Mlp(129, N, 32, batch=4, rms=True, pout=True, rows=(N, 1, 64, N), group="odd"),
                Mlp(127, N, 32, batch=2, rms=False, pout=True, rows=(N, N), bcast=True, group="odd")]
    # per-entry operands
    for N, rms, po in ((256, False, True), (255, True, False), (128, True, True), (192, False, False)):
        out += [Mlp(129, N, 96, batch=4, rms=rms, pout=po, rows=(1, 64, N, 64), npin=3, group="entries"),
                Mlp(129, N, 96, batch=4, rms=rms, pout=po, rows=(N, 1, 64, N), null=3, npin=1, group="entries")]
    out += [Mlp(127, 128, 32, batch=4, rms=False, pout=True, bcast=True, group="entries"),
            Mlp(127, 255, 96, batch=3, rms=False, bcast=True, rows=(255, 1, 64), group="entries")]
    # the 256 x 256 kernel at its smallest: 192 entries of one row tile, and two row tiles with one row in the second
    for M, K, po in itertools.product((1, 257), (32, 64, 96), (False, True)):
        out.append(Mlp(M, 256, K, batch=192, pout=po, group="w256-1" if M == 1 else f"w256-257-{K}"))  # 50 MB each at 257
    out += [Mlp(12033, 256, 32, batch=4, rows=(256, 1, 64, 256), bcast=True, pout=True, group="w256-12033-po"),
            Mlp(12033, 256, 32, batch=4, rows=(256, 256, 256, 256), bcast=True, group="w256-12033")]
    return out


MLP_CASES = _mlp_cases()
CASES = {"f32": F32_CASES, "bf16x3": G3_CASES, "wgrad": WGRAD_CASES, "mlp": MLP_CASES}
BY_NAME = {c.name: c for cs in CASES.values() for c in cs}
assert len(BY_NAME) == sum(len(cs) for cs in CASES.values()), "case names collide"
FAULTS = {"f32": GEMM_FAULTS, "bf16x3": GEMM_FAULTS + SPLIT_FAULTS, "wgrad": SPLIT_FAULTS + RS_FAULTS,
          "mlp": SPLIT_FAULTS + MLP_FAULTS}


def inputs(c):
    return mlp_inputs(c) if isinstance(c, Mlp) else gemm_inputs(c)


def evaluate(c, inp, kind="plain", dt=F64, fault=None):
    return (mlp_eval if isinstance(c, Mlp) else gemm_eval)(c, inp, kind, dt, fault)


# =============================================================================================== refusals
@dataclass(frozen=True)
class Refusal:
    name: str
    entry: str  # "f32" | "bf16x3" | "wgrad" | "wgrad2" | "mlp"
    expect: int
    base: object  # the valid case the refusal starts from
    change: tuple  # (what, value): how the launch departs from the valid case


_RG = G("f32", 40, 40, 64, abi=True)
_RB = G("bf16x3", 64, 64, 64, abi=True)
_RW = G("wgrad", 64, 64, 64, ak=False, bk=False, beta=1.0, bias=0, abi=True)
_RW2 = G("wgrad2", 65, 64, 64, ak=False, bk=False, beta=1.0, bias=0, rs_split=64, abi=True)
_RM = Mlp(65, 128, 32, batch=2, rms=True, pout=True)
_RME = Mlp(65, 128, 32, batch=2, rms=True, pout=True, rows=(128, 64))
_RMEN = Mlp(65, 128, 32, batch=2, rows=(128, 64))  # no input norm: the per-entry batch limit is its own line
REFUSALS = [
    Refusal("f32-null-A", "f32", SD_EARG, _RG, ("null", "A")),
    Refusal("f32-null-C", "f32", SD_EARG, _RG, ("null", "C")),
    Refusal("f32-tile4", "f32", SD_EARG, _RG, ("tile", 4)),
    Refusal("f32-ws-null", "f32", SD_EARG, replace(_RG, ksplit=2), ("ws", None)),
    Refusal("f32-ws-short", "f32", SD_EARG, replace(_RG, ksplit=2), ("ws", -1)),
    Refusal("f32-M0", "f32", SD_OK, _RG, ("dim", ("M", 0))),
    Refusal("f32-N0", "f32", SD_OK, _RG, ("dim", ("N", 0))),
    Refusal("f32-batch0", "f32", SD_OK, _RG, ("dim", ("batch", 0))),
    Refusal("bf16x3-null-B", "bf16x3", SD_EARG, _RB, ("null", "B")),
    Refusal("bf16x3-tile4", "bf16x3", SD_EARG, _RB, ("tile", 4)),
    Refusal("bf16x3-ws-short", "bf16x3", SD_EARG, replace(_RB, ksplit=2), ("ws", -1)),
    Refusal("bf16x3-fallback-ws-short", "bf16x3", SD_EARG, replace(_RB, M=63, ksplit=2), ("ws", -1)),
    Refusal("bf16x3-M0", "bf16x3", SD_OK, _RB, ("dim", ("M", 0))),
    Refusal("wgrad-null-rowsum", "wgrad", SD_EARG, _RW, ("null", "rowsum")),
    Refusal("wgrad-tile4", "wgrad", SD_EARG, _RW, ("tile", 4)),
    Refusal("wgrad-M63", "wgrad", SD_ESHAPE, _RW, ("dim", ("M", 63))),
    Refusal("wgrad-K63", "wgrad", SD_ESHAPE, _RW, ("dim", ("K", 63))),
    Refusal("wgrad-batch0", "wgrad", SD_ESHAPE, _RW, ("dim", ("batch", 0))),
    Refusal("wgrad-batch2", "wgrad", SD_ESHAPE, _RW, ("dim", ("batch", 2))),
    Refusal("wgrad-akcontig", "wgrad", SD_ESHAPE, _RW, ("dim", ("a_kcontig", 1))),
    Refusal("wgrad-ws-short-by-rowsums", "wgrad", SD_EARG, replace(_RW, ksplit=3), ("ws", -1)),
    Refusal("wgrad-ws-slabs-only", "wgrad", SD_EARG, replace(_RW, ksplit=3), ("ws", -3 * 64)),
    Refusal("wgrad-N0", "wgrad", SD_OK, _RW, ("dim", ("N", 0))),
    Refusal("wgrad2-null-rowsum2", "wgrad2", SD_EARG, _RW2, ("null", "rowsum2")),
    Refusal("wgrad2-tile4", "wgrad2", SD_EARG, _RW2, ("tile", 4)),
    Refusal("wgrad2-N63", "wgrad2", SD_ESHAPE, _RW2, ("dim", ("N", 63))),
    Refusal("wgrad2-batch0", "wgrad2", SD_ESHAPE, _RW2, ("dim", ("batch", 0))),
    Refusal("wgrad2-rs0", "wgrad2", SD_ESHAPE, _RW2, ("rs_split", 0)),
    Refusal("wgrad2-rsM", "wgrad2", SD_ESHAPE, _RW2, ("rs_split", 65)),
    Refusal("wgrad2-ws-short-by-rowsums", "wgrad2", SD_EARG, replace(_RW2, ksplit=3), ("ws", -1)),
    Refusal("mlp-null-ext", "mlp", SD_EARG, _RM, ("null", "x")),
    Refusal("mlp-null-C", "mlp", SD_EARG, _RM, ("null", "C")),
    Refusal("mlp-M0", "mlp", SD_OK, _RM, ("dim", ("M", 0))),
    Refusal("mlp-a-rows-contig", "mlp", SD_ESHAPE, _RM, ("dim", ("a_kcontig", 0))),
    Refusal("mlp-b-rows-contig", "mlp", SD_ESHAPE, _RM, ("dim", ("b_kcontig", 0))),
    Refusal("mlp-K-not-32s", "mlp", SD_ESHAPE, _RM, ("dim", ("K", 28))),
    Refusal("mlp-N-below-64", "mlp", SD_ESHAPE, _RM, ("dim", ("N", 63))),
    Refusal("mlp-beta", "mlp", SD_ESHAPE, _RM, ("dim", ("beta", 1.0))),
    Refusal("mlp-lda-odd", "mlp", SD_ESHAPE, _RM, ("dim", ("lda", 33))),
    Refusal("mlp-strideB-odd", "mlp", SD_ESHAPE, _RM, ("dim", ("strideB", 128 * 32 + 1))),
    Refusal("mlp-no-part-in", "mlp", SD_EARG, _RM, ("ext", ("part_in", None))),
    Refusal("mlp-npart-0", "mlp", SD_EARG, _RM, ("ext", ("npart_in", 0))),
    Refusal("mlp-norm-w-stride", "mlp", SD_EARG, _RM, ("ext", ("stride_norm_w", 33))),
    Refusal("mlp-entry-norm-w-missing", "mlp", SD_EARG, _RME, ("ext_entry", ("norm_w_ptr", 1, None))),
    Refusal("mlp-pout-N-not-64s", "mlp", SD_ESHAPE, _RM, ("dim", ("N", 100))),
    Refusal("mlp-pout-stride-short", "mlp", SD_EARG, _RM, ("ext", ("stride_part_out", 2 * 65 - 1))),
    Refusal("mlp-w-rows-negative", "mlp", SD_EARG, _RME, ("ext_entry", ("w_rows", 1, -1))),
    Refusal("mlp-w-rows-above-N", "mlp", SD_EARG, _RME, ("ext_entry", ("w_rows", 1, 129))),
    Refusal("mlp-w-ptr-misaligned", "mlp", SD_ESHAPE, _RME, ("ext_entry", ("w_ptr", 1, "+1"))),
    Refusal("mlp-entries-batch-5", "mlp", SD_EARG, _RMEN, ("dim", ("batch", 5))),
]
