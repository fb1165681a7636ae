// Channels-last (NHWC) convolution as implicit GEMM on the shared MFMA core, plus the conv kernels of the conv
// encoder/decoder with the pooling/norm stage fused into their epilogue. The stage's stand-alone row kernels
// (max-pool + RMSNorm + SiLU forward and backward, FiLM gradients) and their entries are in poolnorm.hip.
//
// Reference: Conv2dSamePad (networks.py:59-85; stride 1, TF-SAME padding), ConvEncoder layers
// [conv -> MaxPool2d(2) -> RMSNorm2D -> SiLU] (networks.py:192-234), ConvDecoder layers
// [Upsample(2, nearest) -> conv -> RMSNorm2D -> SiLU] (networks.py:237-310).
// Layout: activations NHWC (the reference image is already (B,T,H,W,C); RMSNorm2D normalises channels, which
// is a contiguous row in NHWC). Weights are kept as (Co, kh, kw, Ci) so W is a K-contiguous GEMM operand.
//   fwd:        out[m=(n,y,x)][co]      = sum_k im2col(m, k=(ky,kx,ci)) W[co][k] (+ bias)
//   bwd-data:   the same kernel on dOut with the flipped/transposed weight Wf[ci][ky][kx][co], pad' = k-1-pad
//   bwd-weight: dW[co][k]  = sum_m dOut[m][co] im2col(m, k)   (+ a ones column -> d bias), split-K over pixels
// `ups = 1` reads the input through a nearest 2x upsample (decoder) without materialising it.
#include <stdlib.h>

#include "gemm3_core.h"
#include "gemm6_core.h"
#include "gemm_core.h"
#include "sdhip.h"
#include "stage_core.h"

namespace {
using namespace sdg;

struct Geom {
  const float* in;
  int Nb, Hs, Ws, C;  // stored input
  int Hg, Wg;         // conv grid (= Hs<<ups, Ws<<ups)
  int kh, kw, pad, ups;
};

SD_DEV bool tap(const Geom& G, int n, int y, int x, int k, long& off) {
  const int t = k / G.C, c = k - t * G.C;
  const int ky = t / G.kw, kx = t - ky * G.kw;
  const int yy = y + ky - G.pad, xx = x + kx - G.pad;
  if (yy < 0 || yy >= G.Hg || xx < 0 || xx >= G.Wg) return false;
  off = (((long)n * G.Hs + (yy >> G.ups)) * G.Ws + (xx >> G.ups)) * G.C + c;
  return true;
}

// A operand of fwd / bwd-data: rows = output pixels, k = (ky, kx, ci) contiguous in ci.
template <int ROWS, bool VEC>
struct Im2colRows {
  static constexpr int NV = (ROWS * BK / 4 + 255) / 256;
  Geom G;
  int pn[NV], py[NV], px[NV];
  f32x4 r[NV];
  TileLoader<ROWS, true, false> st;  // only for store()
  SD_DEV Im2colRows(const Geom& g, int M, int row0) : G(g) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int i = threadIdx.x + v * 256;
      const int m = row0 + i / (BK / 4);
      pn[v] = -1;
      if (i < ROWS * BK / 4 && m < M) {
        const int hw = G.Hg * G.Wg;
        pn[v] = m / hw;
        const int rem = m - pn[v] * hw;
        py[v] = rem / G.Wg;
        px[v] = rem - py[v] * G.Wg;
      }
    }
  }
  SD_DEV void load(int k0, int kend) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int i = threadIdx.x + v * 256;
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      const int gk = k0 + 4 * (i % (BK / 4));
      if (pn[v] >= 0) {
        if (VEC) {  // C % 16 == 0: the 4 k's share one (ky, kx)
          long off;
          if (gk < kend && tap(G, pn[v], py[v], px[v], gk, off)) x = *reinterpret_cast<const f32x4*>(G.in + off);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            long off;
            if (gk + j < kend && tap(G, pn[v], py[v], px[v], gk + j, off)) x[j] = G.in[off];
          }
        }
      }
      st.r[v] = x;
    }
  }
  SD_DEV void store(float* lds) const { st.store(lds); }
};

// B operand of bwd-weight: rows = j = (ky, kx, ci) (+ one ones-row at j == J for the bias), k = pixel.
template <int ROWS, bool VEC>
struct Im2colCols {
  static constexpr int NV = (ROWS * BK / 4 + 255) / 256;
  Geom G;
  int J, row0;
  TileLoader<ROWS, false, false> st;
  SD_DEV Im2colCols(const Geom& g, int J_, int row0_) : G(g), J(J_), row0(row0_) {}
  SD_DEV void load(int k0, int kend) {
    const int hw = G.Hg * G.Wg;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int i = threadIdx.x + v * 256;
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      const int m = k0 + i % BK;
      const int j0 = row0 + 4 * (i / BK);
      if (i < ROWS * BK / 4 && m < kend) {
        const int n = m / hw, rem = m - n * hw;
        const int y = rem / G.Wg, xq = rem - y * G.Wg;
        if (VEC && j0 + 3 < J) {
          long off;
          if (tap(G, n, y, xq, j0, off)) x = *reinterpret_cast<const f32x4*>(G.in + off);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int jj = j0 + j;
            long off;
            if (jj < J) {
              if (tap(G, n, y, xq, jj, off)) x[j] = G.in[off];
            } else if (jj == J) {
              x[j] = 1.f;
            }
          }
        }
      }
      st.r[v] = x;
    }
  }
  SD_DEV void store(float* lds) const { st.store(lds); }
};

// ---------------------------------------------------------------- tap-table loaders (C % 4 == 0, pow2 grid)
// The k -> (ky, kx, ci) decode of the implicit-GEMM A operand is table-driven: each workgroup writes one packed
// int per 4 k's into LDS (ci | ky << 16 | kx << 24) before its first tile, so a float4 of the im2col row costs an
// LDS read, two compares and an address instead of two runtime integer divisions.
constexpr int MAX_TAPQ = 512;  // K <= 2048
constexpr int NW_D = 8;        // waves of the direct bwd-weight kernel

SD_DEV void build_taps(int* tab, const Geom& G, int K) {
  for (int kq = threadIdx.x; kq < K / 4; kq += blockDim.x) {
    const int k = 4 * kq, t = k / G.C, c = k - t * G.C;
    const int ky = t / G.kw, kx = t - ky * G.kw;
    tab[kq] = c | (ky << 16) | (kx << 24);
  }
  __syncthreads();
}

template <int ROWS>
struct Im2colRowsT {
  static constexpr int NV = (ROWS * BK / 4 + 255) / 256;
  Geom G;
  const int* tab;
  int py[NV], px[NV];
  long pbase[NV];  // n * Hs (row index base) or -1
  TileLoader<ROWS, true, false> st;
  SD_DEV Im2colRowsT(const Geom& g, const int* tab_, int M, int row0, int lw, int lhw) : G(g), tab(tab_) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int i = threadIdx.x + v * 256;
      const int m = row0 + i / (BK / 4);
      pbase[v] = -1;
      if (i < ROWS * BK / 4 && m < M) {
        const int n = m >> lhw, rem = m & ((1 << lhw) - 1);
        py[v] = rem >> lw;
        px[v] = rem & ((1 << lw) - 1);
        pbase[v] = (long)n * G.Hs;
      }
    }
  }
  SD_DEV void load(int k0, int kend) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int i = threadIdx.x + v * 256;
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      const int gk = k0 + 4 * (i % (BK / 4));
      if (pbase[v] >= 0 && gk < kend) {
        const int e = tab[gk >> 2];
        const int yy = py[v] + ((e >> 16) & 0xff) - G.pad, xx = px[v] + (e >> 24) - G.pad;
        if (yy >= 0 && yy < G.Hg && xx >= 0 && xx < G.Wg)
          x = *reinterpret_cast<const f32x4*>(G.in + ((pbase[v] + (yy >> G.ups)) * G.Ws + (xx >> G.ups)) * G.C +
                                              (e & 0xffff));
      }
      st.r[v] = x;
    }
  }
  SD_DEV void store(float* lds) const { st.store(lds); }
};

// Branch-free variant of Im2colRowsT on buffer loads (out-of-image taps and the K tail read 0 through the
// descriptor's range check), for gemm16_mainloop_es. Input must be < 2 GiB (checked by the launcher).
template <int ROWS>
struct Im2colRowsB {
  static constexpr int NV = (ROWS * BK / 4 + 255) / 256;
  Geom G;
  const int* tab;
  sd_rsrc rs;
  int py[NV], px[NV], pb[NV];  // pb: n * Hs, or a large negative value for rows past M
  TileLoader<ROWS, true, false> st;
  SD_DEV Im2colRowsB(const Geom& g, const int* tab_, int M, int row0, int lw, int lhw) : G(g), tab(tab_) {
    rs = sd_make_rsrc(g.in, (long)g.Nb * g.Hs * g.Ws * g.C * 4);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int i = threadIdx.x + v * 256;
      const int m = row0 + i / (BK / 4);
      const int n = m >> lhw, rem = m & ((1 << lhw) - 1);
      py[v] = rem >> lw;
      px[v] = rem & ((1 << lw) - 1);
      pb[v] = (i < ROWS * BK / 4 && m < M) ? n * G.Hs : -(1 << 28);
    }
  }
  SD_DEV void load(int k0, int kend) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int i = threadIdx.x + v * 256;
      const int gk = k0 + 4 * (i % (BK / 4));
      const int e = tab[min(gk >> 2, MAX_TAPQ - 1)];
      const int yy = py[v] + ((e >> 16) & 0xff) - G.pad, xx = px[v] + (e >> 24) - G.pad;
      const bool ok = pb[v] >= 0 && gk < kend && (unsigned)yy < (unsigned)G.Hg && (unsigned)xx < (unsigned)G.Wg;
      const uint32_t off = (uint32_t)((((pb[v] + (yy >> G.ups)) * G.Ws + (xx >> G.ups)) * G.C + (e & 0xffff)) * 4);
      st.r[v] = sd_bload4(rs, ok ? off : SD_OOB);
    }
  }
  SD_DEV void store(float* lds) const { st.store(lds); }
};

// Branch-free dense operand, k contiguous, ROWS x BK tiles of a (nrows x K) matrix with K % 4 == 0 (buffer loads)
template <int ROWS>
struct DenseKCB {
  static constexpr int NV = (ROWS * BK / 4 + 255) / 256;
  sd_rsrc rs;
  long ld;
  int nrows, row0;
  TileLoader<ROWS, true, false> st;
  SD_DEV DenseKCB(const float* base, long ld_, int nrows_, int row0_) : ld(ld_), nrows(nrows_), row0(row0_) {
    rs = sd_make_rsrc(base, (long)nrows_ * ld_ * 4);
  }
  SD_DEV void load(int k0, int kend) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int i = threadIdx.x + v * 256;
      const int row = row0 + i / (BK / 4), gk = k0 + 4 * (i % (BK / 4));
      const bool ok = i < ROWS * BK / 4 && row < nrows && gk < kend;
      st.r[v] = sd_bload4(rs, ok ? (uint32_t)((row * ld + gk) * 4) : SD_OOB);
    }
  }
  SD_DEV void store(float* lds) const { st.store(lds); }
};

// fwd / bwd-data: M = pixels, N = Co (tile = all output channels), 16x16x4 MFMA, 4 waves along M
template <int BN, bool ES>
__global__ __launch_bounds__(256) void conv_fwd16(GemmArgs g, Geom G, int lw, int lhw) {
  __shared__ int tab[MAX_TAPQ];
  build_taps(tab, G, g.K);
  constexpr int BM = 128;
  const int bm0 = blockIdx.x * BM;
  if constexpr (ES) {
    Im2colRowsB<BM> la(G, tab, g.M, bm0, lw, lhw);
    DenseKCB<BN> lb(g.B, g.ldb, g.N, 0);
    gemm_block16<BM, BN, 32, BN, true>(g, la, lb, bm0, 0, 0, 0, 0, g.K);
  } else {
    Im2colRowsT<BM> la(G, tab, g.M, bm0, lw, lhw);
    DenseOperand<BN, true, true> lb(g.B, g.ldb, g.N, 0);
    gemm_block16<BM, BN, 32, BN>(g, la, lb, bm0, 0, 0, 0, 0, g.K);
  }
}

// Stage epilogue shared by the fused forward kernels: the 128-pixel conv tile (+ bias) is staged in LDS at C, 2x2
// max-pooled (argmax kept for the backward), RMS-normalised over the BN channels (8 threads per pooled pixel) and
// SiLU'd; only the pooled outputs are written (pooled pre-norm values, argmax, rstd; y NHWC or NCHW-flat).
// pre (optional): the caller's registers holding this lane's bias values (BN / 16: column 16 j + l16) and norm
// weights (BN / 8: channel t8 + 8 k), loaded once per workgroup — in a kernel with loads in flight at the epilogue
// (a prefetched next patch) the per-tile loads here would each wait for them too (vmcnt counts in issue order).
template <int BN>
struct EpiPre {
  float bias[BN / 16];
  float nw[BN / 8];
};
// NW, the stage's norm weight (`const float*`, or FilmNW for the FiLM stage): stage_core.h
template <int BN, int WM, class NW>
SD_DEV void pool_epilogue(const f32x4 (&acc)[WM / 16][BN / 16], float* C, const GemmArgs& g, const Geom& G, int lw,
                          int lhw, int bm0, NW nw, float* pooled, uint8_t* amax, float* y, float* rstd,
                          float eps, int nchw_flat, const EpiPre<BN>* pre = nullptr) {
  constexpr int LDC = BN + 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, q = lane >> 4;
#pragma unroll
  for (int i = 0; i < WM / 16; ++i)
#pragma unroll
    for (int j = 0; j < BN / 16; ++j) {
      const int col = 16 * j + l16;
      const float bv = pre ? pre->bias[j] : g.bias ? g.bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) C[(wave * WM + 16 * i + 4 * q + r) * LDC + col] = acc[i][j][r] + bv;
    }
  __syncthreads();
  constexpr int NK = BN / 8;
  // WM / 32 passes of (threads / 8) pooled pixels x 8 threads (a wave's WM pixels hold WM / 4 pooled ones)
#pragma unroll
  for (int ps = 0; ps < WM / 32; ++ps) {
  const int tid = threadIdx.x, pp = (tid >> 3) + ps * (int)(blockDim.x >> 3), t8 = tid & 7;
  const int W = G.Wg, Wo = W >> 1, lwo = lw - 1;
  const int yo = pp >> lwo, xo = pp & (Wo - 1);
  const int l0 = (2 * yo) * W + 2 * xo;                     // local pixel of the window's top-left
  const int gp = bm0 + l0;                                    // global conv pixel
  const int n = gp >> lhw, rem = gp & ((1 << lhw) - 1), yy = rem >> lw, xx = rem & (W - 1);
  const int Ho = G.Hg >> 1;
  const long gpp = ((long)n * Ho + (yy >> 1)) * Wo + (xx >> 1);  // global pooled pixel
  const bool valid = gp < g.M;
  float v[NK];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int c = t8 + 8 * k;
    float best = -INFINITY;
    int bi = 0;
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const float val = C[(l0 + (qd >> 1) * W + (qd & 1)) * LDC + c];
      if (val > best || isnan(val)) { best = val; bi = qd; }
    }
    v[k] = best;
    ss += best * best;
    if (valid) {
      pooled[gpp * BN + c] = best;
      amax[gpp * BN + c] = (uint8_t)bi;
    }
  }
  ss = group_sum<8>(ss);
  const float r = rsqrtf(ss / (float)BN + eps);
  if (valid && t8 == 0) rstd[gpp] = r;
  const long prem = gpp - (long)n * Ho * Wo;
  long fo = 0;  // FiLM: this pixel's context row (row 0 for a pixel past the last image: nothing is stored for it)
  if constexpr (is_film<NW>) fo = (long)(valid ? n / nw.ipc : 0) * BN;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int c = t8 + 8 * k;
    float z = v[k] * r * (pre ? pre->nw[k] : nw_of(nw)[c]);
    if constexpr (is_film<NW>) z = nw.gamma[fo + c] * z + nw.beta[fo + c];
    const long o = nchw_flat ? (long)n * BN * Ho * Wo + (long)c * Ho * Wo + prem : gpp * BN + c;
    if (valid) y[o] = siluf_(z);
  }
  }
}


// ConvEncoder stage fused: conv (fwd16 main loop) -> MaxPool2d(2) -> RMSNorm2D -> SiLU (networks.py:201-216).
// A 128-pixel M tile holds whole 2x2 windows (128 % 2W == 0, image rows come in pairs), so the epilogue stages the
// conv tile in the main loop's LDS area, pools it, normalises over the Co channels (8 threads per pooled pixel) and
// writes only the pooled outputs (pooled pre-norm values, argmax, rstd for the backward; y NHWC or NCHW-flat).
template <int BN, bool ES, class NW = const float*>
__global__ __launch_bounds__(256) void conv_fwd16_pool(GemmArgs g, Geom G, int lw, int lhw, NW nw,
                                                       float* pooled, uint8_t* amax, float* y, float* rstd, float eps,
                                                       int nchw_flat) {
  __shared__ int tab[MAX_TAPQ];
  build_taps(tab, G, g.K);
  constexpr int BM = 128, WM = 32;
  const int bm0 = blockIdx.x * BM;
  EpiPre<BN> pre;  // epilogue operands issued ahead of the main loop (no loads behind the epilogue's own stores)
#pragma unroll
  for (int j = 0; j < BN / 16; ++j) pre.bias[j] = g.bias ? g.bias[16 * j + (threadIdx.x & 15)] : 0.f;
#pragma unroll
  for (int k = 0; k < BN / 8; ++k) pre.nw[k] = nw_of(nw)[(threadIdx.x & 7) + 8 * k];
  f32x4 acc[WM / 16][BN / 16];
  if constexpr (ES) {
    Im2colRowsB<BM> la(G, tab, g.M, bm0, lw, lhw);
    DenseKCB<BN> lb(g.B, g.ldb, g.N, 0);
    gemm16_mainloop_es<BM, BN, WM, BN>(la, lb, 0, g.K, acc);
  } else {
    Im2colRowsT<BM> la(G, tab, g.M, bm0, lw, lhw);
    DenseOperand<BN, true, true> lb(g.B, g.ldb, g.N, 0);
    gemm16_mainloop<BM, BN, WM, BN>(la, lb, 0, g.K, acc);
  }
  __syncthreads();  // every wave is done reading the staging area
  float* C = sd_smem<gemm16_smem_floats<BM, BN>()>();
  static_assert(BM * (BN + 1) <= gemm16_smem_floats<BM, BN>(), "tile fits the staging area");
  pool_epilogue<BN, WM>(acc, C, g, G, lw, lhw, bm0, nw, pooled, amax, y, rstd, eps, nchw_flat, &pre);
}

// Direct ConvEncoder stage forward (stride 1, same padding, no upsample): the 128-pixel tile is R = 128 / W whole
// output rows of one image, so its receptive field is one (R + KS - 1) x (W + KS - 1) x CI input patch. The patch
// is staged in LDS once (pixel stride CI + 4 floats: conflict-free ds_read_b128 fragments) and every tap's A
// fragments are read from it at the tap's offset — the 25x im2col expansion is never re-read from L2. The weights
// stream through a double-buffered early-store B stage, one (tap, 32-channel) k tile per iteration; the epilogue
// (pool + RMSNorm + SiLU) is conv_fwd16_pool's, staged in the patch area. Wave w owns tile pixels 32w..32w+31
// (TM = 2) x all BN channels. One tile per workgroup, in XCD-aware order: an XCD's workgroups cover a contiguous tile
// range, so the KS - 1 halo rows adjacent tiles share are L2 hits. (Workgroups running 2 or 4 vertically adjacent
// tiles, the next tile's patch loaded into registers under the current tile's MFMAs, were built and not kept.)
template <int BN, int CI, int LW, int KS, class NW = const float*>
__global__ __launch_bounds__(256) void conv_fwd_direct_pool(GemmArgs g, Geom G, int lhw, NW nw,
                                                            float* pooled, uint8_t* amax, float* y, float* rstd,
                                                            float eps, int nchw_flat) {
  constexpr int BM = 128, WM = 32, TM = WM / 16, TN = BN / 16, W = 1 << LW, R = BM / W;
  constexpr int PH = R + KS - 1, PW = W + KS - 1, CSI = CI + 4, PAD = KS / 2;
  constexpr int PATCH = PH * PW * CSI, SB = BN * LDS_ROW;
  constexpr int NQ = PH * PW * (CI / 4), NQT = (NQ + 255) / 256;
  constexpr int NK = KS * KS * (CI / BK);
  static_assert(CI % 32 == 0 && (CSI / 4) % 2 == 1, "32-channel k tiles, odd float4 pixel stride");
  static_assert(BM * (BN + 1) <= PATCH, "epilogue tile fits the patch area");
  float* smem = sd_smem<PATCH + 2 * SB>();
  float* patch = smem;
  float* bst = smem + PATCH;
  const int nwg = gridDim.x, ntiles = g.M / BM;
  const int wg = (nwg & 7) ? blockIdx.x : (blockIdx.x & 7) * (nwg >> 3) + (blockIdx.x >> 3);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, q = lane >> 4;
  const sd_rsrc rs = sd_make_rsrc(G.in, (long)G.Nb * G.Hs * G.Ws * CI * 4);
  f32x4 v[NQT];
  auto load_patch = [&](int tile) {  // zero outside the image (range-checked buffer loads)
    const int bm0 = tile * BM, n = bm0 >> lhw, y0 = (bm0 & ((1 << lhw) - 1)) >> LW;
#pragma unroll
    for (int u = 0; u < NQT; ++u) {
      const int i = threadIdx.x + 256 * u;
      const int pix = i / (CI / 4), c4 = i % (CI / 4);
      const int py = pix / PW, px = pix % PW;
      const int yy = y0 + py - PAD, xx = px - PAD;
      const bool ok = i < NQ && tile < ntiles && (unsigned)yy < (unsigned)G.Hs && (unsigned)xx < (unsigned)W;
      v[u] = sd_bload4(rs, ok ? (uint32_t)((((n * G.Hs + yy) * W + xx) * CI + 4 * c4) * 4) : SD_OOB);
    }
  };
  // fragment base of tile pixel p = 32w + 16i + l16 (row p >> LW, column p & (W - 1)) at tap (0, 0)
  int abase[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int p = wave * WM + 16 * i + l16;
    abase[i] = ((p >> LW) * PW + (p & (W - 1))) * CSI + 8 * q;
  }
  DenseKCB<BN> lb(g.B, g.ldb, g.N, 0);
  const int tile = wg;
  load_patch(tile);
  if (tile >= ntiles) return;  // uniform over the workgroup
  lb.load(0, g.K);
#pragma unroll
  for (int u = 0; u < NQT; ++u) {
    const int i = threadIdx.x + 256 * u;
    if ((u + 1) * 256 <= NQ || i < NQ)
      *reinterpret_cast<f32x4*>(patch + (i / (CI / 4)) * CSI + 4 * (i % (CI / 4))) = v[u];
  }
  lb.store(bst);
  lb.load(BK, g.K);
  __syncthreads();
  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kt = 0; kt < NK; ++kt) {
    const float* cur = bst + (kt & 1) * SB;
    float* nxt = bst + ((kt & 1) ^ 1) * SB;
    const int tap = kt / (CI / BK), ci0 = (kt % (CI / BK)) * BK;
    const int toff = ((tap / KS) * PW + tap % KS) * CSI + ci0;
    float af[TM][8], bf[TN][8];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const float* pa = patch + abase[i] + toff;
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(pa), x1 = *reinterpret_cast<const f32x4*>(pa + 4);
#pragma unroll
      for (int s = 0; s < 4; ++s) { af[i][s] = x0[s]; af[i][4 + s] = x1[s]; }
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const float* pb = cur + (16 * j + l16) * LDS_ROW + 8 * q;
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(pb), x1 = *reinterpret_cast<const f32x4*>(pb + 4);
#pragma unroll
      for (int s = 0; s < 4; ++s) { bf[j][s] = x0[s]; bf[j][4 + s] = x1[s]; }
    }
    lb.store(nxt);
    lb.load((kt + 2 < NK ? kt + 2 : NK - 1) * BK, g.K);
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][s], bf[j][s], acc[i][j], 0, 0, 0);
    __syncthreads();
  }
  pool_epilogue<BN, WM>(acc, patch, g, G, LW, lhw, tile * BM, nw, pooled, amax, y, rstd, eps, nchw_flat);
}

// conv_fwd_direct_pool on the fp32-accurate three-way split-bf16 path (gemm6_core.h: a = a0 + a1 + a2, six
// v_mfma_f32_16x16x32_bf16 per 32-deep k chunk, smallest terms first, <= 2^-26 |ab| dropped per product; 2.67x the
// f32 MFMA rate). The 128-pixel tile's input patch is staged once, split into three bf16 planes (pixel stride CI + 8
// bf16: conflict-free ds_read_b128 fragments), and every tap reads its shifted window from there; the weight comes
// pre-split ([plane][BN][KP] bf16, sd_conv_split3_weight) straight from L2, one k chunk ahead. A lane's 8 k values of
// a chunk are 8 consecutive channels of one tap (CI % 8 == 0), so CI need not be a multiple of 32. Wave w owns tile
// pixels 32w..32w+31 (two 16-pixel tiles) x all BN channels; the epilogue (pool + RMSNorm + SiLU) is
// conv_fwd16_pool's, staged in the patch area.
template <int BN, int CI, int LW, int KS, class NW = const float*>
__global__ __launch_bounds__(256, 2) void conv_fwd6_direct_pool(GemmArgs g, Geom G, int lhw,
                                                                 const __bf16* __restrict__ wsp, NW nw,
                                                                 float* pooled, uint8_t* amax, float* y, float* rstd,
                                                                 float eps, int nchw_flat) {
  constexpr int W = 1 << LW, R = 128 / W, PH = R + KS - 1, PW = W + KS - 1, CP = CI + 8, PAD = KS / 2;
  constexpr int PLANE = PH * PW * CP, K = KS * KS * CI, NKC = (K + 31) / 32, KP = NKC * 32, TN = BN / 16;
  constexpr int CI4 = CI / 4, NEL = PH * PW * CI4, NE = (NEL + 255) / 256;
  static_assert(CI % 8 == 0 && 128 % W == 0 && BN % 16 == 0, "geometry");
  static_assert(128 * (BN + 1) * 4 <= 3 * PLANE * 2, "epilogue tile fits the patch area");
  typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
  extern __shared__ __attribute__((aligned(16))) __bf16 patch6[];  // [plane][PH][PW][CP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q = lane >> 4;
  const int bm0 = blockIdx.x * 128, n = bm0 >> lhw, y0 = (bm0 & ((1 << lhw) - 1)) >> LW;
  {
    f32x4 v[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int i = tid + 256 * e, c4 = i % CI4, pix = i / CI4, pc = pix % PW, pr = pix / PW;
      const int yy = y0 + pr - PAD, xx = pc - PAD;
      v[e] = (i < NEL && (unsigned)yy < (unsigned)G.Hs && (unsigned)xx < (unsigned)W)
                 ? *reinterpret_cast<const f32x4*>(G.in + (((long)n * G.Hs + yy) * W + xx) * CI + 4 * c4)
                 : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int i = tid + 256 * e;
      if (i < NEL) {
        const int c4 = i % CI4, pix = i / CI4;
        float h0, h1, h2, h3, m0, m1, m2, m3;
        const u32x2 h{bf16_pair(v[e][0], v[e][1], h0, h1), bf16_pair(v[e][2], v[e][3], h2, h3)};
        const float r0 = v[e][0] - h0, r1 = v[e][1] - h1, r2 = v[e][2] - h2, r3 = v[e][3] - h3;
        const u32x2 m{bf16_pair(r0, r1, m0, m1), bf16_pair(r2, r3, m2, m3)};
        const f32x4 l{r0 - m0, r1 - m1, r2 - m2, r3 - m3};
        __bf16* dst = patch6 + pix * CP + 4 * c4;
        *reinterpret_cast<u32x2*>(dst) = h;
        *reinterpret_cast<u32x2*>(dst + PLANE) = m;
        *reinterpret_cast<bf16x4*>(dst + 2 * PLANE) = __builtin_convertvector(l, bf16x4);
      }
    }
  }
  int pbase[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int p = 32 * wave + 16 * mt + l16;
    pbase[mt] = ((p >> LW) * PW + (p & (W - 1))) * CP;
  }
  const __bf16* wl = wsp + (long)l16 * KP + 8 * q;
  bf16x8 b[2][TN][3];
  auto bload = [&](int kc, int s) {
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
        b[s][j][pl] = *reinterpret_cast<const bf16x8*>(wl + ((long)pl * BN + 16 * j) * KP + 32 * kc);
  };
  f32x4 acc[2][TN];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bload(0, 0);
  __syncthreads();
  auto chunk = [&](int kc, int s) {
    if (kc + 1 < NKC) bload(kc + 1, s ^ 1);
    int k0 = 32 * kc + 8 * q;
    k0 = k0 < K ? k0 : K - 8;  // past K: any in-patch address (the weight is zero there)
    const int tap = k0 / CI, c0 = k0 - tap * CI, ky = tap / KS, kx = tap - ky * KS;
    const int off = (ky * PW + kx) * CP + c0;
    bf16x8 a[2][3];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) a[mt][pl] = *reinterpret_cast<const bf16x8*>(patch6 + pl * PLANE + pbase[mt] + off);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        f32x4 c = acc[mt][j];
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt][2], b[s][j][0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt][1], b[s][j][1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt][0], b[s][j][2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt][1], b[s][j][0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt][0], b[s][j][1], c, 0, 0, 0);
        acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt][0], b[s][j][0], c, 0, 0, 0);
      }
  };
  int kc = 0;
  for (; kc + 2 <= NKC; kc += 2) {
    chunk(kc, 0);
    chunk(kc + 1, 1);
  }
  if (kc < NKC) chunk(kc, 0);
  __syncthreads();  // every wave is done reading the patch
  pool_epilogue<BN, 32>(acc, reinterpret_cast<float*>(patch6), g, G, LW, lhw, bm0, nw, pooled, amax, y, rstd, eps,
                        nchw_flat);
}

// conv_fwd6_direct_pool with the weight through LDS (round 6): 256-pixel tiles on 512-thread workgroups, the input
// patch staged once as three bf16 planes (as there), and the pre-split weight staged per 32-deep k chunk into a
// double-buffered LDS ring shared by the 8 waves (conv_dgrad3_direct's ring, three planes) instead of every lane loading
// its own fragments from L2 (0.9 MB of weight per 128-pixel tile: the L2 -> CU path bound the kernel, MFMA busy 0.37).
// Same products in the same k order: bit-identical to conv_fwd6_direct_pool.
// The patch planes are channel-group-major ([plane][CI / 8][PH * PW][8] bf16), not pixel-major with a pad: the 16
// lanes of a fragment read 16 consecutive pixels' 16-B pieces (conflict-free with no pad), so the 48 -> 64 stage's
// whole-image 256-pixel tile (20 x 20 x 48 patch) fits beside the ring (146 KB; pixel-major with its pad was 165 KB).
// (The 32 -> 48 stage ran pixel-major on 256-pixel tiles until its 512-pixel tiles, below, took the same layout.)
// Tried and retired: a fragment register pipeline (chunk kc + 1's fragments read from LDS into a second register set
// under chunk kc's MFMAs, so that the LDS read latency was not exposed once per chunk) measured 1 % faster alone
// (profiles/r06s3b) but spilled together with the patch prefetch, and lost to the multi-tile workgroups.
// TPW: a workgroup runs TPW consecutive tiles (XCD-contiguous ranges, so the halo rows adjacent tiles share are L2
// hits), the next tile's patch loaded into registers under this tile's MFMAs and the ring's first chunk under its
// epilogue: with one workgroup per CU the prologue's HBM round trip was otherwise exposed once per tile.
// MT: 16-pixel m tiles per wave (2: 256-pixel tiles; 4: 512-pixel tiles, each wave 64 pixels x BN channels — 21
// fragment reads per 72 MFMAs instead of 15 per 36: less LDS traffic per product). BROW: the ring's row stride in bf16
// (40 = 32 + a pad; 32 = packed, the 64-B rows of a fragment read are still 1 KB contiguous).
// 512 threads (the 48 -> 64 stage's whole image as four 64-pixel waves on 256 threads measured slower than eight
// 32-pixel waves, 213.7 vs 180.5 us, profiles/r06m3: one wave per SIMD).
template <int BN, int CI, int LW, int KS, int TPW, int MT = 2, int BROW = 40, class NW = const float*>
__global__ __launch_bounds__(512, 1) void conv_fwd6r_direct_pool(GemmArgs g, Geom G, int lhw,
                                                                  const __bf16* __restrict__ wsp, NW nw,
                                                                  float* pooled, uint8_t* amax, float* y, float* rstd,
                                                                  float eps, int nchw_flat) {
  constexpr int NTH = 512, TP = 16 * MT * (NTH / 64);
  constexpr int W = 1 << LW, R = TP / W, PH = R + KS - 1, PW = W + KS - 1, PAD = KS / 2;
  constexpr int NPIX = PH * PW, PLANE = NPIX * CI, K = KS * KS * CI, NKC = (K + 31) / 32, KP = NKC * 32, TN = BN / 16;
  constexpr int CI4 = CI / 4, NEL = PH * PW * CI4, NE = (NEL + NTH - 1) / NTH;
  constexpr int SB = 3 * BN * BROW, NPC = 3 * BN * 4, NPT = (NPC + NTH - 1) / NTH;  // ring: [plane][n][BROW]
  // element offset of (pixel, channel c, c % 4 == 0) in a plane
  auto poff = [](int pix, int c) { return ((c >> 3) * NPIX + pix) * 8 + (c & 7); };
  static_assert(CI % 8 == 0 && TP % W == 0 && BN % 16 == 0, "geometry");
  static_assert(TP * (BN + 1) * 4 <= 3 * PLANE * 2, "epilogue tile fits the patch area");
  typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
  extern __shared__ __attribute__((aligned(16))) __bf16 patch6r[];  // [plane][CI / 8][NPIX][8], then the ring [2][SB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q = lane >> 4;
  const int nwg = gridDim.x, ntiles = g.M / TP;
  const int wg = (nwg & 7) ? blockIdx.x : (blockIdx.x & 7) * (nwg >> 3) + (blockIdx.x >> 3);
  __bf16* bst = patch6r + 3 * PLANE;
  bf16x8 br[NPT];
  auto bload = [&](int kc) {  // piece i: plane i / (4 BN), row (i / 4) % BN, 16-B piece i % 4 of the chunk
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int i = tid + NTH * u;
      if (i < NPC) br[u] = *reinterpret_cast<const bf16x8*>(wsp + (long)(i >> 2) * KP + 32 * kc + 8 * (i & 3));
    }
  };
  auto bstore = [&](int st) {
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int i = tid + NTH * u;
      if (i < NPC) *reinterpret_cast<bf16x8*>(bst + st * SB + (i >> 2) * BROW + 8 * (i & 3)) = br[u];
    }
  };
  f32x4 v[NE];
  auto load_patch = [&](int tile) {
    const int bm0 = tile * TP, n = bm0 >> lhw, y0 = (bm0 & ((1 << lhw) - 1)) >> LW;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int i = tid + NTH * e, c4 = i % CI4, pix = i / CI4, pc = pix % PW, pr = pix / PW;
      const int yy = y0 + pr - PAD, xx = pc - PAD;
      v[e] = (i < NEL && tile < ntiles && (unsigned)yy < (unsigned)G.Hs && (unsigned)xx < (unsigned)W)
                 ? *reinterpret_cast<const f32x4*>(G.in + (((long)n * G.Hs + yy) * W + xx) * CI + 4 * c4)
                 : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto store_patch = [&]() {
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int i = tid + NTH * e;
      if (i < NEL) {
        const int c4 = i % CI4, pix = i / CI4;
        float h0, h1, h2, h3, m0, m1, m2, m3;
        const u32x2 h{bf16_pair(v[e][0], v[e][1], h0, h1), bf16_pair(v[e][2], v[e][3], h2, h3)};
        const float r0 = v[e][0] - h0, r1 = v[e][1] - h1, r2 = v[e][2] - h2, r3 = v[e][3] - h3;
        const u32x2 m{bf16_pair(r0, r1, m0, m1), bf16_pair(r2, r3, m2, m3)};
        const f32x4 l{r0 - m0, r1 - m1, r2 - m2, r3 - m3};
        __bf16* dst = patch6r + poff(pix, 4 * c4);
        *reinterpret_cast<u32x2*>(dst) = h;
        *reinterpret_cast<u32x2*>(dst + PLANE) = m;
        *reinterpret_cast<bf16x4*>(dst + 2 * PLANE) = __builtin_convertvector(l, bf16x4);
      }
    }
  };
  int pbase[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int p = 16 * MT * wave + 16 * mt + l16;
    pbase[mt] = (p >> LW) * PW + (p & (W - 1));  // pixel index at tap (0, 0)
  }
  bload(0);
  load_patch(wg * TPW);
  for (int it = 0; it < TPW; ++it) {
  const int tile = wg * TPW + it;
  if (tile >= ntiles) break;  // uniform over the workgroup
  if (it > 0) __syncthreads();  // the previous tile's epilogue is done with the patch area
  store_patch();
  bstore(0);
  if (NKC > 1) bload(1);
  f32x4 acc[MT][TN];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  if (it + 1 < TPW) load_patch(tile + 1);
  for (int kc = 0; kc < NKC; ++kc) {
    const __bf16* bs = bst + (kc & 1) * SB + l16 * BROW + 8 * q;
    bf16x8 b[TN][3];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) b[j][pl] = *reinterpret_cast<const bf16x8*>(bs + (pl * BN + 16 * j) * BROW);
    int k0 = 32 * kc + 8 * q;
    k0 = k0 < K ? k0 : K - 8;  // past K: any in-patch address (the weight is zero there)
    const int tap = k0 / CI, c0 = k0 - tap * CI, ky = tap / KS, kx = tap - ky * KS;
    const int toff = ky * PW + kx;
    bf16x8 a[MT][3];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
        a[mt][pl] = *reinterpret_cast<const bf16x8*>(patch6r + pl * PLANE + poff(pbase[mt] + toff, c0));
    if (kc + 1 < NKC) bstore((kc + 1) & 1);  // chunk kc + 1 (loaded one iteration ago) into the other stage
    if (kc + 2 < NKC) bload(kc + 2);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        f32x4 c = acc[mt][j];
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt][2], b[j][0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt][1], b[j][1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt][0], b[j][2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt][1], b[j][0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt][0], b[j][1], c, 0, 0, 0);
        acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt][0], b[j][0], c, 0, 0, 0);
      }
    __syncthreads();
  }
  if (it + 1 < TPW) bload(0);  // the next tile's first weight chunk (the same weights) under the epilogue
  pool_epilogue<BN, 16 * MT>(acc, reinterpret_cast<float*>(patch6r), g, G, LW, lhw, tile * TP, nw, pooled, amax, y,
                             rstd, eps, nchw_flat);
  }
}

// [plane][n][KP] three-way split-bf16 image (gemm6_core.h split) of a (rows, K) fp32 matrix, zero past K
__global__ __launch_bounds__(256) void split3_weight(const float* __restrict__ w, __bf16* __restrict__ out, int rows,
                                                     int K, int KP) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)rows * KP) return;
  const int r = (int)(i / KP), k = (int)(i % KP);
  const float v = k < K ? w[(long)r * K + k] : 0.f;
  const __bf16 a0 = (__bf16)v;
  const float r1 = v - (float)a0;
  const __bf16 a1 = (__bf16)r1;
  const long pl = (long)rows * KP;
  out[i] = a0;
  out[pl + i] = a1;
  out[2 * pl + i] = (__bf16)(r1 - (float)a1);
}

// Direct forward for the 4-channel (padded RGB) first stage: K = 25 taps x 4 channels, so one
// v_mfma_f32_16x16x4_f32 step is exactly one tap (lane (l16, q) supplies channel q of pixel l16's tap sample) and
// nothing is padded to a 32-wide k tile. The whole weight (BN x 100 floats) lives in registers (each lane keeps its
// 25 x TN fragments, loaded once per workgroup), the (R + KS - 1) x (W + KS - 1) x 4 input patch in LDS (one
// float4 per pixel: the b32 fragment reads of 64 lanes hit 64 distinct banks). A workgroup runs TPW vertically
// adjacent tiles (XCD-aware: an XCD's workgroups cover a contiguous tile range), prefetching the next tile's patch
// into registers under the current tile's MFMAs; the epilogue is conv_fwd16_pool's, in its own LDS area.
// tpw (runtime) tiles per workgroup: the launcher sizes the grid to one round of resident workgroups (OCC per CU),
// so no partial last round of long workgroups idles part of the chip.
template <int BN, int LW, int KS, int OCC, class NW = const float*>
__global__ __launch_bounds__(256, OCC) void conv_fwd_direct_pool_c4(GemmArgs g, Geom G, int lhw, int TPW,
                                                                    NW nw, float* pooled, uint8_t* amax,
                                                                    float* y, float* rstd, float eps, int nchw_flat) {
  constexpr int BM = 128, WM = 32, TM = WM / 16, TN = BN / 16, W = 1 << LW, R = BM / W;
  constexpr int PH = R + KS - 1, PW = W + KS - 1, PAD = KS / 2, NT = KS * KS;
  constexpr int NQ = PH * PW, NQT = (NQ + 255) / 256;
  // the patch area is padded to NQT * 256 pixels, so every thread's staging store is unconditional (a store under a
  // branch left the compiler a path on which the loop-invariant weight loads looked outstanding: it then waited for
  // the next tile's prefetch, vmcnt(0), before the first MFMA of every tile)
  float* smem = sd_smem<NQT * 256 * 4 + BM * (BN + 1)>();
  float* patch = smem;
  float* C = smem + NQT * 256 * 4;
  const int nwg = gridDim.x, ntiles = g.M / BM;
  const int wg = (nwg & 7) ? blockIdx.x : (blockIdx.x & 7) * (nwg >> 3) + (blockIdx.x >> 3);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, q = lane >> 4;
  float bw[NT][TN];
  {
    const sd_rsrc rb = sd_make_rsrc(g.B, (long)g.N * g.ldb * 4);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < TN; ++j) bw[t][j] = sd_bload1(rb, (uint32_t)(((16 * j + l16) * g.ldb + 4 * t + q) * 4));
  }
  EpiPre<BN> pre;
#pragma unroll
  for (int j = 0; j < TN; ++j) pre.bias[j] = g.bias ? g.bias[16 * j + l16] : 0.f;
#pragma unroll
  for (int k = 0; k < BN / 8; ++k) pre.nw[k] = nw_of(nw)[(threadIdx.x & 7) + 8 * k];
  const sd_rsrc rs = sd_make_rsrc(G.in, (long)G.Nb * G.Hs * G.Ws * 16);
  f32x4 v[NQT];
  auto load_patch = [&](int tile) {
    const int bm0 = tile * BM, n = bm0 >> lhw, y0 = (bm0 & ((1 << lhw) - 1)) >> LW;
#pragma unroll
    for (int u = 0; u < NQT; ++u) {
      const int i = threadIdx.x + 256 * u;
      const int py = i / PW, px = i % PW;
      const int yy = y0 + py - PAD, xx = px - PAD;
      const bool ok = i < NQ && tile < ntiles && (unsigned)yy < (unsigned)G.Hs && (unsigned)xx < (unsigned)W;
      v[u] = sd_bload4(rs, ok ? (uint32_t)(((n * G.Hs + yy) * W + xx) * 16) : SD_OOB);
    }
  };
  int abase[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int p = wave * WM + 16 * i + l16;
    abase[i] = ((p >> LW) * PW + (p & (W - 1))) * 4 + q;
  }
  load_patch(wg * TPW);
  for (int it = 0; it < TPW; ++it) {
    const int tile = wg * TPW + it;
    if (tile >= ntiles) break;  // uniform over the workgroup
#pragma unroll
    for (int u = 0; u < NQT; ++u) *reinterpret_cast<f32x4*>(patch + 4 * (threadIdx.x + 256 * u)) = v[u];
    __syncthreads();  // patch staged (and the previous tile's epilogue is past its C reads)
    if (it + 1 < TPW) load_patch(tile + 1);
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int toff = ((t / KS) * PW + t % KS) * 4;
      float a[TM];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = patch[abase[i] + toff];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bw[t][j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();  // every wave is done reading the patch before the next tile's is stored
    pool_epilogue<BN, WM>(acc, C, g, G, LW, lhw, tile * BM, nw, pooled, amax, y, rstd, eps, nchw_flat, &pre);
  }
}

// (A variant of conv_fwd_direct_pool streaming each lane's weight fragments into registers, with no LDS stage, no
// barriers and 3 workgroups per CU, measured slower: 679 vs 660 us on encoder stage 2 at 1024 images.)

// ---------------------------------------------------------------- direct bwd-weight (stride 1, no upsample)
// dW[co][j = (ky,kx,ci)] (+ d bias at j = J) = sum over pixels of dy[p][co] * x[p + (ky,kx) - pad][ci].
// A 512-thread workgroup stages one block of R image rows in LDS — the dy rows (R*W x Co) and the input patch with
// its halo ((R+kh-1) x (W+kw-1) x Ci, zero padded) — and runs every (co, j) product of that block from LDS, so the
// 25x im2col expansion is never read from memory (one patch read per row block instead of one per tap).
// Wave w owns NBW 16-column blocks of j, all TM 16-row blocks of co: acc = TM*NBW 16x16 fp32 tiles in registers,
// accumulated over the row blocks blockIdx.y, +gridDim.y, ...; the gridDim.y partial slabs are summed by slab_reduce.
// One skeleton (wgrad_direct_body) on two math paths, WdF32 and WdBf16x3: a path keeps its LDS layout and one-time
// initialisation, its dy fetch registers and stage, its patch stage and the contraction over a staged block.
struct DirectW {
  const float* x;
  const float* dy;      // (Nb, H, W, Co) conv-output gradient, or (PL) the pooled-resolution gradient (Nb, H/2, W/2, Co)
  const uint8_t* amax;  // PL: the 2x2 max-pool argmax per pooled element (dy is routed to that window position)
  float* ws;
  int Nb, H, W, Ci, Co, kh, kw, pad, R, lw;  // lw = log2(W)
  int J, PW, PH, CP, DS, blocks;  // DS: stride of the staged dy (f32: floats per pixel; split-bf16: bf16 per channel)
};

constexpr int WD_VA = 4, WD_VP = 6;  // max float4 per thread of a staged dy block (f32 path) / input patch

// column j < J = (ky, kx, ci): its tap's pixel shift + its channel, in elements of a [PH][PW][CP] patch image
SD_DEV int wd_tap_off(const DirectW& d, int j) {
  const int t = j / d.Ci, ci = j - t * d.Ci, ky = t / d.kw, kx = t - ky * d.kw;
  return (ky * d.PW + kx) * d.CP + ci;
}

// The f32 path. MFMA 16x16x4: lane (l16, q) supplies dy[p = 4s+q][co = l16] and x-patch[p = 4s+q][j = l16].
// LDS row strides are padded to 16 (mod 64) floats so the 4 lane groups hit distinct banks.
template <int TM, bool PL>
struct WdF32 {
  const DirectW& d;
  const int tid, nA;
  float* const dyl;  // [P][DS]
  float* const xp;   // [PH][PW][CP]; channel Ci holds 1.0 (bias column), Ci+1 holds 0.0
  f32x4 ra[WD_VA];
  uint32_t aa[PL ? WD_VA : 1];
  SD_DEV WdF32(const DirectW& d_, float* lds, int tid_)
      : d(d_), tid(tid_), nA(d_.R * d_.W * d_.Co / 4), dyl(lds), xp(lds + d_.R * d_.W * d_.DS) {}
  SD_DEV void init() {  // the constant channels never change: write them once
    for (int pix = tid; pix < d.PH * d.PW; pix += 512) {
      xp[pix * d.CP + d.Ci] = 1.f;
      xp[pix * d.CP + d.Ci + 1] = 0.f;
    }
  }
  // this lane's column of the block starting at j0 (j == J -> the ones channel, j > J -> the zero channel)
  SD_DEV int col_off(int j0, int l16) const {
    const int j = j0 + l16;
    return j < d.J ? wd_tap_off(d, j) : d.Ci + (j == d.J ? 0 : 1);
  }
  SD_DEV void fetch_dy(int n, int y0) {
    const float* dsrc = d.dy + ((long)n * d.H + y0) * d.W * d.Co;
#pragma unroll
    for (int v = 0; v < WD_VA; ++v) {
      const int i = tid + 512 * v;
      if constexpr (PL) {  // item i = (pooled pixel of the block, 4-channel group): raw gradient + argmax bytes
        ra[v] = f32x4{0.f, 0.f, 0.f, 0.f};
        aa[v] = 0xffffffffu;
        if (i < nA / 4) {
          const long pp = (((long)n * (d.H >> 1) + (y0 >> 1)) * (d.W >> 1)) * d.Co + 4 * i;
          ra[v] = *reinterpret_cast<const f32x4*>(d.dy + pp);
          aa[v] = *reinterpret_cast<const uint32_t*>(d.amax + pp);
        }
      } else {
        ra[v] = i < nA ? *reinterpret_cast<const f32x4*>(dsrc + 4 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }
  SD_DEV void stage_dy() {
#pragma unroll
    for (int v = 0; v < WD_VA; ++v) {
      const int i = tid + 512 * v;
      if constexpr (PL) {  // route the pooled gradient to its argmax position of the 2x2 window, zeros elsewhere
        if (i < nA / 4) {
          const int e = 4 * i, pl = e / d.Co, c = e - pl * d.Co;
          const int hw = d.W >> 1, pr = pl / hw, pc = pl - pr * hw;
#pragma unroll
          for (int qd = 0; qd < 4; ++qd) {
            const int p = (2 * pr + (qd >> 1)) * d.W + 2 * pc + (qd & 1);
            f32x4 val;
#pragma unroll
            for (int k = 0; k < 4; ++k) val[k] = ((aa[v] >> (8 * k)) & 0xffu) == (uint32_t)qd ? ra[v][k] : 0.f;
            *reinterpret_cast<f32x4*>(dyl + p * d.DS + c) = val;
          }
        }
      } else if (i < nA) {
        const int e = 4 * i, p = e / d.Co, c = e - p * d.Co;
        *reinterpret_cast<f32x4*>(dyl + p * d.DS + c) = ra[v];
      }
    }
  }
  SD_DEV void settle_dy() {}
  SD_DEV void stage_patch(int pix, int c, const f32x4& v) { *reinterpret_cast<f32x4*>(xp + pix * d.CP + c) = v; }
  template <int NBW, bool WS>
  SD_DEV void contract(f32x4 (&acc)[TM][NBW], const int (&off)[NBW], int P, int wave, int l16, int q) {
    for (int s = WS ? wave : 0; s < P / 4; s += WS ? NW_D : 1) {
      const int p = 4 * s + q, py = p >> d.lw, px = p & (d.W - 1);
      float a[TM];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = dyl[p * d.DS + 16 * i + l16];
      const float* xb = xp + (py * d.PW + px) * d.CP;
      float bv[NBW];
#pragma unroll
      for (int b = 0; b < NBW; ++b) bv[b] = xb[off[b]];
#pragma unroll
      for (int b = 0; b < NBW; ++b)
#pragma unroll
        for (int i = 0; i < TM; ++i) acc[i][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bv[b], acc[i][b], 0, 0, 0);
    }
  }
};

// The split-bf16 path, on v_mfma_f32_16x16x32_bf16 (~1e-5 relative, three products per step).
// k = pixels, 32 per MFMA step: lane group q supplies pixels 4i + q (i = 0..7) of the step. dy of the block is staged
// transposed and pre-split, [co][pos] per plane with pos = 8 (p % 4) + (p / 4) % 8 inside each 32-pixel step, so a
// lane's 8 A-values are one ds_read_b128 per plane (rows >= Co read zero rows).
// The input patch is staged PRE-SPLIT as two bf16 planes, hi and lo (split2's values), each [PH][PW][CP] with the
// channels contiguous, and the B operand comes from transposed reads: per column block and plane two
// ds_read_b64_tr_b16, each a 4-pixel x 16-column block per 16-lane group, delivered column-major. In group q, lane
// 4 r + c (r, c = 0..3) supplies the address of pixel 4 r + q (second read: 4 (r + 4) + q) of the step, shifted by
// the tap of column quad 16 b + 4 c, at that quad's first channel; lane l16 receives column 16 b + l16 of the 4
// pixels, so the two reads are the lane's k = 0..3 and 4..7: the operands of the word-gather form this replaces (8
// ds_read_b32 and 4 v_perm_b32 per column block), in the same slots, bit for bit. A quad never straddles a tap
// (Ci % 4 == 0 and a block starts at a multiple of 16), though a block may span several (Ci = 4: four; Ci = 24).
// The constant channels are the quad [1, 0, 0, 0] at Ci .. Ci + 3 (column J is the bias column). Quads past J read
// that quad as well: B column n reaches only column n of the tile, and no column past J is stored.
// What the transposed read asks for: every lane's address 8-byte aligned (CP, Ci and every channel offset are
// multiples of 4 elements, the plane bases multiples of 8 bytes), and EXEC all ones (512 threads, a k loop whose
// bounds are scalar, no lane-dependent branch around the reads: every lane reads an in-bounds quad).
// Banks ((a / 4) % 64 per 32-lane half = two neighbouring pixels x 4 pixels x 4 quads): 2-way at CP = 16 or 48
// (mod 64) elements, the floor of any pixel stride for this k -> pixel assignment.
template <int TM, bool PL, bool WSK = false>  // WSK: a wave-split rung (only its pooled-gradient fetch differs)
struct WdBf16x3 {
  typedef __attribute__((address_space(3))) sdb::bf16x4 lds_bf16x4;
  const DirectW& d;
  const int tid;
  __bf16* const xh;   // [PH][PW][CP], the hi plane; channels Ci .. Ci+3 hold [1, 0, 0, 0]
  __bf16* const xl;   // the lo plane, behind it (the constant quad is [0, 0, 0, 0] here)
  __bf16* const dyh;  // [TM*16][DS]
  __bf16* const dyl;
  // this thread's dy block: 4 channels x 4 pixels (pixels c + 4 (4 ih + t) of 32-pixel step sb, t = 0..3)
  int nD, dq4, dc, dih, dsb;  // nD 4x4 blocks: 8 pixel groups per 32-pixel step
  f32x4 rd[4];
  uint32_t aw[PL ? 4 : 1];  // PL: the 4 channels' argmax bytes of each pixel's pooled element
  int dy0;                  // PL: the fetched block's first image row (its parity places a pixel in its 2x2 window)
  SD_DEV WdBf16x3(const DirectW& d_, float* lds, int tid_)
      : d(d_), tid(tid_), xh(reinterpret_cast<__bf16*>(lds)), xl(xh + d_.PH * d_.PW * d_.CP),
        dyh(reinterpret_cast<__bf16*>(lds + d_.PH * d_.PW * d_.CP)), dyl(dyh + TM * 16 * d_.DS) {
    for (int e = tid; e < TM * 16 * d.DS; e += 512) {  // rows >= Co stay zero; rows < Co are overwritten per block
      dyh[e] = (__bf16)0.f;
      dyl[e] = (__bf16)0.f;
    }
  }
  SD_DEV void init() {  // the thread's dy block and the constant channels
    const int c4 = d.Co / 4, drest = tid / c4;
    nD = c4 * (d.R * d.W / 4);
    dq4 = tid % c4;
    dc = drest % 4, dih = (drest / 4) % 2, dsb = drest / 8;
    sdb::bf16x4 one, zero;
    sdb::split2(f32x4{1.f, 0.f, 0.f, 0.f}, one, zero);
    for (int pix = tid; pix < d.PH * d.PW; pix += 512) {
      *reinterpret_cast<sdb::bf16x4*>(xh + pix * d.CP + d.Ci) = one;
      *reinterpret_cast<sdb::bf16x4*>(xl + pix * d.CP + d.Ci) = zero;
    }
  }
  // byte offset, from a pixel of a plane, of the quad this lane addresses in the column block starting at column j0
  SD_DEV int col_off(int j0, int l16) const {
    const int j = j0 + 4 * (l16 & 3);
    return 2 * (j < d.J ? wd_tap_off(d, j) : d.Ci);
  }
  SD_DEV void fetch_dy(int n, int y0) {
    [[maybe_unused]] const float* dsrc = d.dy + ((long)n * d.H + y0) * d.W * d.Co;
    // PL, not WS: the block's first pooled row is a workgroup-uniform base and a pixel's pooled element a 32-bit offset
    // from it ((y0 + r) / 2 == y0 / 2 + r / 2 for every row r of the block: R is even, and y0 with it, or R is 1),
    // recomputed per block (px made opaque) instead of hoisted: as 64-bit element indices from d.dy the offsets kept 14
    // loop-invariant registers live across the MFMA loop, and the <3, 7> rung then reloaded a spilled pointer between
    // the two groups of loads, a full wait for the first group before the second was issued (+ 8 % on that launch).
    // The wave-split first-stage rungs have the registers and little MFMA work to hide the recomputation under (it
    // cost them 185 -> 223 us at 1,024 images): they keep the hoisted 64-bit form.
    [[maybe_unused]] const long pbase = (((long)n * (d.H >> 1) + (y0 >> 1)) * (d.W >> 1)) * d.Co;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      int px = 32 * dsb + dc + 4 * (4 * dih + t);
      if constexpr (PL) {  // the pooled element of pixel px (row y0 + px / W), loaded whole; masked in stage_dy()
        long pp;
        if constexpr (WSK) {
          const int yy = y0 + (px >> d.lw), xx = px & (d.W - 1);
          pp = (((long)n * (d.H >> 1) + (yy >> 1)) * (d.W >> 1) + (xx >> 1)) * d.Co + 4 * dq4;
        } else {
          asm volatile("" : "+v"(px));
          pp = pbase + ((((px >> d.lw) >> 1) * (d.W >> 1) + ((px & (d.W - 1)) >> 1)) * d.Co + 4 * dq4);
        }
        const bool ok = tid < nD;
        rd[t] = ok ? *reinterpret_cast<const f32x4*>(d.dy + pp) : f32x4{0.f, 0.f, 0.f, 0.f};
        aw[t] = ok ? *reinterpret_cast<const uint32_t*>(d.amax + pp) : 0xffffffffu;
        dy0 = y0;
      } else {
        rd[t] = tid < nD ? *reinterpret_cast<const f32x4*>(dsrc + (long)px * d.Co + 4 * dq4)
                         : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }
  // PL: route the pooled gradient to its argmax position of the 2x2 window, zeros elsewhere
  SD_DEV void mask_dy() {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int px = 32 * dsb + dc + 4 * (4 * dih + t);  // the pixel's position in its 2x2 window: row, column parity
      const uint32_t qd = (uint32_t)(((dy0 + (px >> d.lw)) & 1) * 2 + (px & 1));
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (((aw[t] >> (8 * k)) & 0xffu) != qd) rd[t][k] = 0.f;
    }
  }
  // Called after a block's MFMAs (and after the first fetch): the pooled form masks the fetched block here, in
  // registers, while other waves still run their MFMAs, instead of between the two barriers of stage_dy, where every
  // wave waits (the 32 compares and selects per thread there cost the <3, 7> rung what the smaller fetch gained it).
  // The wave-split rungs, a single MFMA step per wave and block, keep the mask in stage_dy.
  SD_DEV void settle_dy() {
    if constexpr (PL && !WSK) mask_dy();
  }
  SD_DEV void stage_dy() {
    if (tid < nD) {
      const int pos = 32 * dsb + 8 * dc + 4 * dih;
      if constexpr (PL && WSK) mask_dy();
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const f32x4 t = {rd[0][jj], rd[1][jj], rd[2][jj], rd[3][jj]};
        sdb::bf16x4 hi, lo;
        sdb::split2(t, hi, lo);
        const int o = (4 * dq4 + jj) * d.DS + pos;
        *reinterpret_cast<sdb::bf16x4*>(dyh + o) = hi;
        *reinterpret_cast<sdb::bf16x4*>(dyl + o) = lo;
      }
    }
  }
  SD_DEV void stage_patch(int pix, int c, const f32x4& v) {
    sdb::bf16x4 hi, lo;
    sdb::split2(v, hi, lo);
    *reinterpret_cast<sdb::bf16x4*>(xh + pix * d.CP + c) = hi;
    *reinterpret_cast<sdb::bf16x4*>(xl + pix * d.CP + c) = lo;
  }
  static SD_DEV sdb::bf16x8 tr_pair(uint32_t a0, uint32_t a1) {  // two transposed reads: a lane's k = 0..3 | 4..7
    const sdb::bf16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(reinterpret_cast<lds_bf16x4*>(a0));
    const sdb::bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(reinterpret_cast<lds_bf16x4*>(a1));
    return __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
  }
  template <int NBW, bool WS>
  SD_DEV void contract(f32x4 (&acc)[TM][NBW], const int (&off)[NBW], int P, int wave, int l16, int q) {
    // LDS byte addresses (the low half of a shared pointer's flat address is its LDS offset)
    const uint32_t xh0 = (uint32_t)reinterpret_cast<uintptr_t>(xh), plane = 2u * d.PH * d.PW * d.CP;
    const int s0 = WS ? __builtin_amdgcn_readfirstlane(wave) : 0;  // a scalar loop: EXEC stays all ones
    for (int s = s0; s < P / 32; s += WS ? NW_D : 1) {
      sdb::bf16x8 ah[TM], al[TM];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int o = (16 * i + l16) * d.DS + 32 * s + 8 * q;
        ah[i] = *reinterpret_cast<const sdb::bf16x8*>(dyh + o);
        al[i] = *reinterpret_cast<const sdb::bf16x8*>(dyl + o);
      }
      uint32_t pa[2];  // the hi plane's address of this lane's pixel row of each read
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int p = 32 * s + 4 * ((l16 >> 2) + 4 * r) + q, py = p >> d.lw, px = p & (d.W - 1);
        pa[r] = xh0 + 2u * ((py * d.PW + px) * d.CP);
      }
#pragma unroll
      for (int b = 0; b < NBW; ++b) {
        const sdb::bf16x8 bh = tr_pair(pa[0] + off[b], pa[1] + off[b]);
        const sdb::bf16x8 bl = tr_pair(pa[0] + off[b] + plane, pa[1] + off[b] + plane);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          acc[i][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh, acc[i][b], 0, 0, 0);
          acc[i][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl, acc[i][b], 0, 0, 0);
          acc[i][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh, acc[i][b], 0, 0, 0);
        }
      }
    }
  }
};

// WS (wave split): for narrow j ranges (the 4-channel first stage: J + 1 = 101 -> 7 blocks) every wave covers all j
// blocks over every 8th k step, and the 8 waves' tiles are summed through LDS at the end.
// PL: dy is the max-pool backward's input (pooled resolution + argmax, sd_pool_rms_bwd_compact of poolnorm.hip),
// expanded while it is fetched — the full-resolution conv gradient (3/4 zeros) is never written to or read from HBM.
template <class M, int TM, int NBW, bool WS>
SD_DEV void wgrad_direct_body(const DirectW& d) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, q = lane >> 4;
  const int P = d.R * d.W;
  M m(d, lds, tid);
  // per-lane decode of this wave's j blocks: the f32 path's column, the split-bf16 path's column quad
  int off[NBW];
#pragma unroll
  for (int b = 0; b < NBW; ++b) off[b] = m.col_off(16 * (WS ? b : (blockIdx.x * NW_D + wave) * NBW + b), l16);
  f32x4 acc[TM][NBW];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int b = 0; b < NBW; ++b) acc[i][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int rows_per_img = d.H / d.R, cq = d.Ci / 4, nP = d.PH * d.PW * cq;
  f32x4 rp[WD_VP];
  // global -> registers for row block rb (all loads issued together)
  auto fetch = [&](int rb) {
    const int n = rb / rows_per_img, y0 = (rb - n * rows_per_img) * d.R;
    m.fetch_dy(n, y0);
#pragma unroll
    for (int v = 0; v < WD_VP; ++v) {
      const int i = tid + 512 * v;
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      if (i < nP) {
        const int pix = i / cq, c = 4 * (i - pix * cq);
        const int py = pix / d.PW, px = pix - py * d.PW;
        const int iy = y0 - d.pad + py, ix = px - d.pad;
        if (iy >= 0 && iy < d.H && ix >= 0 && ix < d.W)
          x = *reinterpret_cast<const f32x4*>(d.x + (((long)n * d.H + iy) * d.W + ix) * d.Ci + c);
      }
      rp[v] = x;
    }
  };
  auto stage = [&]() {
    m.stage_dy();
#pragma unroll
    for (int v = 0; v < WD_VP; ++v) {
      const int i = tid + 512 * v;
      if (i < nP) {
        const int pix = i / cq, c = 4 * (i - pix * cq);
        m.stage_patch(pix, c, rp[v]);
      }
    }
  };
  m.init();
  int rb = blockIdx.y;
  if (rb < d.blocks) {
    fetch(rb);
    m.settle_dy();
  }
  for (; rb < d.blocks; rb += gridDim.y) {
    __syncthreads();  // previous block's LDS reads are done
    stage();
    __syncthreads();
    const bool more = rb + (int)gridDim.y < d.blocks;
    if (more) fetch(rb + gridDim.y);  // next block's loads overlap this block's MFMAs
    m.template contract<NBW, WS>(acc, off, P, wave, l16, q);
    if (more) m.settle_dy();
  }
  // partial slab blockIdx.y: ws[split][co][J+1]
  float* out = d.ws + (long)blockIdx.y * d.Co * (d.J + 1);
  if constexpr (WS) {  // sum the 8 waves' tiles through LDS (the staging area is free now), one 16x16 tile at a time
#pragma unroll
    for (int b = 0; b < NBW; ++b)
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) lds[(wave * 4 + r) * 64 + lane] = acc[i][b][r];
        __syncthreads();
        if (tid < 256) {
          const int r = tid >> 6, ln = tid & 63;
          float v = 0.f;
#pragma unroll
          for (int w = 0; w < NW_D; ++w) v += lds[(w * 4 + r) * 64 + ln];
          const int j = 16 * b + (ln & 15), co = 16 * i + 4 * (ln >> 4) + r;
          if (j <= d.J && co < d.Co) out[(long)co * (d.J + 1) + j] = v;
        }
      }
    return;
  }
#pragma unroll
  for (int b = 0; b < NBW; ++b) {
    const int j = 16 * ((blockIdx.x * NW_D + wave) * NBW + b) + l16;
    if (j <= d.J) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = 16 * i + 4 * q + r;
          if (co < d.Co) out[(long)co * (d.J + 1) + j] = acc[i][b][r];
        }
    }
  }
}

template <int TM, int NBW, bool WS, bool PL = false>
__global__ __launch_bounds__(512) void conv_wgrad_direct(DirectW d) {
  wgrad_direct_body<WdF32<TM, PL>, TM, NBW, WS>(d);
}
template <int TM, int NBW, bool WS = false, bool PL = false>
__global__ __launch_bounds__(512) void conv_wgrad3_direct(DirectW d) {
  wgrad_direct_body<WdBf16x3<TM, PL, WS>, TM, NBW, WS>(d);
}

// ---------------------------------------------------------------- split-bf16 backward (gemm3_core.h)
// The two backward contractions of a convolution on the bf16x3 MFMA path (~1e-5 relative, 5.3x the f32 rate):
// only gradients flow through them, no sampled latent depends on them.

// A KC-layout f32 loader (st.r[v]: thread i = tid + 256 v holds row i / 8, k 4 * (i % 8) .. +3) staged as split bf16
template <class L, int ROWS>
struct KCSplit {
  L& l;
  SD_DEV explicit KCSplit(L& l_) : l(l_) {}
  SD_DEV void load(int k0, int kend) { l.load(k0, kend); }
  SD_DEV void store(__bf16* lds) const {
#pragma unroll
    for (int v = 0; v < L::NV; ++v) {
      const int i = threadIdx.x + v * 256;
      if ((v + 1) * 256 <= ROWS * BK / 4 || i < ROWS * BK / 4)
        sdb::split_store(lds + (i / (BK / 4)) * sdb::LROW + 4 * (i % (BK / 4)), l.st.r[v]);
    }
  }
};

// bwd-data: dIn = conv_same(dOut, flipped W) as implicit GEMM, M = pixels (128 per workgroup), N = the input's
// channels (one tile), K = kh*kw*C(dOut); 4 waves along M.
template <int BN>
__global__ __launch_bounds__(256, 2) void conv_dgrad3(GemmArgs g, Geom G, int lw, int lhw) {
  __shared__ int tab[MAX_TAPQ];
  build_taps(tab, G, g.K);
  constexpr int BM = 128;
  const int bm0 = blockIdx.x * BM;
  Im2colRowsB<BM> la0(G, tab, g.M, bm0, lw, lhw);
  DenseKCB<BN> lb0(g.B, g.ldb, g.N, 0);
  KCSplit<Im2colRowsB<BM>, BM> la(la0);
  KCSplit<DenseKCB<BN>, BN> lb(lb0);
  f32x4 acc[2][BN / 16];
  sdb::gemm3_mainloop<BM, BN, 32, BN>(la, lb, 0, g.K, acc);
  epilogue16<BM, BN, 32, BN>(g, acc, bm0, 0, 0, 0);
}

// ---------------------------------------------------------------- wide stages (a channel count above 128)
// The same two contractions tiled over N as well as M, for the shapes the kernels above refuse (Co <= 64 is baked into
// them): any channel counts (154, 231: no multiple of 4), any K (25 * 154 = 3850: past the tap table, no multiple of
// 32). 128 x 64 tiles, 4 waves along M, gemm3_mainloop; M, N and K tails masked by the loaders and by epilogue16.

// A operand of the wide bwd-data: Im2colRows' rows and k order, but no division in the K loop. A thread's first k of a
// tile is kbeg + 32 t + 4 (tid % 8) for all its rows, so its (ky, kx, c) is decoded once and stepped by 32 channels
// per tile; inside a float4 the channel steps by one and wraps into the next tap. VEC: C % 4 == 0 and a 16-B aligned
// base (the four k's share one tap). The main loop asks for the tiles in ascending order. ups = 0.
template <int ROWS, bool VEC>
struct Im2colRowsInc {
  static constexpr int NV = (ROWS * BK / 4 + 255) / 256;
  Geom G;
  int pn[NV], py[NV], px[NV];
  int kcur, c, ky, kx;
  TileLoader<ROWS, true, false> st;  // only for store() (KCSplit reads st.r)
  SD_DEV Im2colRowsInc(const Geom& g, int M, int row0, int kbeg) : G(g) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int i = threadIdx.x + v * 256;
      const int m = row0 + i / (BK / 4);
      pn[v] = -1;
      if (i < ROWS * BK / 4 && m < M) {
        const int hw = G.Hg * G.Wg;
        pn[v] = m / hw;
        const int rem = m - pn[v] * hw;
        py[v] = rem / G.Wg;
        px[v] = rem - py[v] * G.Wg;
      }
    }
    kcur = kbeg + 4 * (threadIdx.x % (BK / 4));
    const int t = kcur / G.C;
    c = kcur - t * G.C;
    ky = t / G.kw;
    kx = t - ky * G.kw;
  }
  SD_DEV bool tap_base(int v, int ty, int tx, long& off) const {
    const int yy = py[v] + ty - G.pad, xx = px[v] + tx - G.pad;
    off = (((long)pn[v] * G.Hs + yy) * G.Ws + xx) * G.C;
    return yy >= 0 && yy < G.Hg && xx >= 0 && xx < G.Wg;
  }
  SD_DEV void load(int k0, int kend) {
    const int gk = k0 + 4 * (threadIdx.x % (BK / 4));
    while (kcur < gk) {
      kcur += BK;
      c += BK;
      while (c >= G.C) {
        c -= G.C;
        if (++kx == G.kw) { kx = 0; ++ky; }
      }
    }
    // every load is issued unconditionally (a masked-off element reads in[0] and is dropped): a load under a branch
    // makes hipcc wait for it at the merge, which serialises the tile's loads
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      const bool row = pn[v] >= 0 && gk < kend;
      long off;
      bool ok = tap_base(v, ky, kx, off) && row;
      if (VEC) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(G.in + (ok ? off + c : 0));
        if (ok) x = t;
      } else {
        int cc = c, ty = ky, tx = kx;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool okj = ok && gk + j < kend;
          const float t = G.in[okj ? off + cc : 0];
          x[j] = okj ? t : 0.f;
          if (++cc == G.C) {
            cc = 0;
            if (++tx == G.kw) { tx = 0; ++ty; }
            ok = tap_base(v, ty, tx, off) && row;
          }
        }
      }
      st.r[v] = x;
    }
  }
};

// B operand of the wide bwd-weight: Im2colCols' rows j = (ky, kx, ci) with the bias ones-row at j == J, k = pixel,
// staged as split bf16. A thread keeps ONE row j for the whole K loop (tid % ROWS, decoded once) and loads four
// consecutive pixels of it per slot: consecutive lanes read consecutive channels of one tap (coalesced), and the four
// pixels are one k-run of the LDS row (one 8-B store per plane, where Im2colCols' layout would need eight 2-B ones).
template <int ROWS>
struct Im2colColsPix {
  static_assert(256 % ROWS == 0, "one row per thread");
  static constexpr int NV = ROWS * BK / 4 / 256;
  Geom G;
  int J, j, ky, kx, c;
  f32x4 r[NV];
  SD_DEV Im2colColsPix(const Geom& g, int J_, int row0) : G(g), J(J_) {
    j = row0 + threadIdx.x % ROWS;
    const int t = j / G.C;
    c = j - t * G.C;
    ky = t / G.kw;
    kx = t - ky * G.kw;
  }
  SD_DEV void load(int k0, int kend) {
    const int hw = G.Hg * G.Wg;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int m0 = k0 + 4 * ((threadIdx.x + v * 256) / ROWS);
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      // (m0 >= kend decodes to pixels past the batch: every element is masked; loads unconditional, as above)
      int n = m0 / hw;
      const int rem = m0 - n * hw;
      int y = rem / G.Wg, xq = rem - y * G.Wg;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool live = m0 + e < kend;
        const int yy = y + ky - G.pad, xx = xq + kx - G.pad;
        const bool in = live && j < J && yy >= 0 && yy < G.Hg && xx >= 0 && xx < G.Wg;
        const float t = G.in[in ? (((long)n * G.Hs + yy) * G.Ws + xx) * G.C + c : 0];
        x[e] = in ? t : (live && j == J ? 1.f : 0.f);
        if (++xq == G.Wg) {
          xq = 0;
          if (++y == G.Hg) { y = 0; ++n; }
        }
      }
      r[v] = x;
    }
  }
  SD_DEV void store(__bf16* lds) const {
#pragma unroll
    for (int v = 0; v < NV; ++v)
      sdb::split_store(lds + (threadIdx.x % ROWS) * sdb::LROW + 4 * ((threadIdx.x + v * 256) / ROWS), r[v]);
  }
};

// gemm3_core.h's two dense operands with every load issued unconditionally (masked-off elements read p[0])
template <int ROWS, bool VEC>
struct KC3U : sdb::KC3<ROWS, VEC> {
  using B = sdb::KC3<ROWS, VEC>;
  using B::B;
  SD_DEV void load(int k0, int kend) {
#pragma unroll
    for (int v = 0; v < B::NV; ++v) {
      const int i = threadIdx.x + v * 256;
      const int row = i / (BK / 4), gk = k0 + 4 * (i % (BK / 4)), gr = this->row0 + row;
      const bool ok = i < ROWS * BK / 4 && gr < this->nrows;
      const long off = (long)gr * this->ld + gk;
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      if (VEC) {  // K % 4 == 0: the four k's are inside together
        const bool okv = ok && gk < kend;
        const f32x4 t = *reinterpret_cast<const f32x4*>(this->p + (okv ? off : 0));
        if (okv) x = t;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool okj = ok && gk + j < kend;
          const float t = this->p[okj ? off + j : 0];
          x[j] = okj ? t : 0.f;
        }
      }
      this->r[v] = x;
    }
  }
};

template <int ROWS, bool VEC>
struct KM3U : sdb::KM3<ROWS, VEC> {
  using B = sdb::KM3<ROWS, VEC>;
  using B::B;
  SD_DEV void load(int k0, int kend) {
#pragma unroll
    for (int v = 0; v < B::NV; ++v) {
      const int i = threadIdx.x + v * 256;
      const int rq = i % (ROWS / 4), kq = i / (ROWS / 4);
      const int gr = this->row0 + 4 * rq;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int gk = k0 + 4 * kq + kk;
        const bool ok = i < B::NBLK && gk < kend;
        const long off = (long)gk * this->ld + gr;
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {  // nrows % 4 == 0: the four rows are inside together
          const bool okv = ok && gr < this->nrows;
          const f32x4 t = *reinterpret_cast<const f32x4*>(this->p + (okv ? off : 0));
          if (okv) x = t;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bool okj = ok && gr + j < this->nrows;
            const float t = this->p[okj ? off + j : 0];
            x[j] = okj ? t : 0.f;
          }
        }
        this->r[v][kk] = x;
      }
    }
  }
};

constexpr int WIDE_BM = 128, WIDE_BN = 64;

// bwd-data: M = pixels, N = dIn's channels in 64-wide tiles, K = kh*kw*C(dOut). Workgroup b: N tile b % ntn of M tile
// b / ntn, so the N tiles of one pixel block run side by side and share its dOut rows in L2.
template <bool VA, bool VB>
__global__ __launch_bounds__(256, 2) void conv_dgrad_wide3(GemmArgs g, Geom G, int ntn) {
  constexpr int BM = WIDE_BM, BN = WIDE_BN;
  const int bn0 = (blockIdx.x % ntn) * BN, bm0 = (blockIdx.x / ntn) * BM;
  Im2colRowsInc<BM, VA> la0(G, g.M, bm0, 0);
  KCSplit<Im2colRowsInc<BM, VA>, BM> la(la0);
  KC3U<BN, VB> lb(g.B, g.ldb, g.N, bn0);
  f32x4 acc[2][BN / 16];
  sdb::gemm3_mainloop<BM, BN, 32, BN>(la, lb, 0, g.K, acc);
  epilogue16<BM, BN, 32, BN>(g, acc, bm0, bn0, 0, 0);
}

// bwd-weight: M = Co in 128-row tiles, N = j (+ the bias column) in 64-wide tiles, K = pixels, split into gridDim.y
// slabs of g.kchunk pixels; every slab goes to the workspace (slab_reduce sums them, one slab included).
template <bool VA>
__global__ __launch_bounds__(256, 2) void conv_wgrad_wide3(GemmArgs g, Geom G, int J, int ntn) {
  constexpr int BM = WIDE_BM, BN = WIDE_BN;
  const int bn0 = (blockIdx.x % ntn) * BN, bm0 = (blockIdx.x / ntn) * BM;
  const int split = blockIdx.y;
  const int kbeg = split * g.kchunk;
  const int kend = min(g.K, kbeg + g.kchunk);
  KM3U<BM, VA> la(g.A, g.lda, g.M, bm0);
  Im2colColsPix<BN> lb(G, J, bn0);
  f32x4 acc[2][BN / 16];
  sdb::gemm3_mainloop<BM, BN, 32, BN>(la, lb, kbeg, kend, acc);
  epilogue16<BM, BN, 32, BN>(g, acc, bm0, bn0, 0, split);
}

// bwd-data as a DIRECT convolution on split-bf16 MFMAs: conv_dgrad3's contraction (dIn = conv_same(dOut, flipped W),
// K = (ky, kx, c) with c contiguous), but each workgroup stages its dOut patch (R image rows + the kh-1 / kw-1 halo,
// zero outside the image) ONCE in LDS, split to (hi, lo) bf16 planes on the way in, and every tap reads its shifted
// window from there: each dOut element is loaded and split once per workgroup instead of once per tap it feeds
// (conv_dgrad3's im2col staging re-split it up to kh*kw times: VALU-bound, 0.2 of the bf16x3 peak). The B operand
// comes pre-split ([plane][n][KP] bf16, sd_conv_split_weight) straight from global memory (L2-resident, 16 B per lane
// per plane), one k chunk ahead. M = R*W output pixels per workgroup (128), 4 waves x 2 16-pixel tiles, NT 16-channel
// tiles of dIn; per 32-deep k chunk a lane's 8 k values are 8 consecutive channels of one tap (CIN % 8 == 0), one
// ds_read_b128 per plane. Products: lo_a*hi_b + hi_a*lo_b + hi_a*hi_b (gemm3_mainloop's order), f32 accumulation.
// Round 6: MT = 4 16-pixel m tiles per wave over NTHR threads (the tile is 64 NTHR / 64 pixels), the patch
// channel-group-major ([plane][CIN / 8][pixel][8]: no pad, conflict-free), as conv_fwd6r_direct_pool's 64-pixel
// waves: 12 fragment reads per 24 MFMAs instead of 8 per 12. Same products in the same k order. The first form, 128-pixel
// tiles of 32-pixel waves (MT = 2) with a padded pixel-major patch, two workgroups per CU, was retired: 183 -> 131 us
// alone on the 64 -> 48 stage (profiles/r06dg3).
// PL: dout is the max-pool backward's pooled-resolution gradient (Nb, H / 2, W / 2, CIN) and amax the forward's argmax
// bytes (sd_pool_rms_bwd_compact, poolnorm.hip): the full-resolution dOut (3/4 zeros) exists only in the LDS patch.
// A thread's item is one pooled element x 4 channels of the pooled rows / columns whose 2x2 windows touch the patch
// (any parity of the patch's first row and column): one f32x4 + 4 argmax bytes loaded, one split, and each of the window's four positions
// inside the patch written with the value where the channel's argmax names the position and zero elsewhere. The
// windows tile the plane, so every patch slot is written exactly once (pooled indices outside the image write zeros)
// with the bits the full-resolution form stages there: same products, same k order, the same dIn bit for bit.
template <int CIN, int NT, int LW, int KS, int NTHR, bool PL = false>
__global__ __launch_bounds__(NTHR, 2) void conv_dgrad3_direct(const float* __restrict__ dout,
                                                               const uint8_t* __restrict__ amax,
                                                               const __bf16* __restrict__ wsp, float* __restrict__ din,
                                                               int Nb, int H, int pad) {
  constexpr int MT = 4, TP = 16 * MT * (NTHR / 64);
  constexpr int W = 1 << LW, R = TP / W, PH = R + KS - 1, PW = W + KS - 1, NPIX = PH * PW;
  constexpr int PLANE = NPIX * CIN, K = KS * KS * CIN, NKC = (K + 31) / 32, KP = NKC * 32, NOUT = 16 * NT;
  constexpr int CIN4 = CIN / 4, NEL = PH * PW * CIN4, NE = (NEL + NTHR - 1) / NTHR;
  static_assert(CIN % 8 == 0 && R >= 1 && TP % W == 0, "geometry");
  // element offset of (pixel, channel c, c % 4 == 0) in a plane
  auto poff = [](int pix, int c) { return ((c >> 3) * NPIX + pix) * 8 + (c & 7); };
  extern __shared__ __attribute__((aligned(16))) __bf16 patch[];  // [plane][CIN / 8][NPIX][8]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q = lane >> 4;
  const int rows_per_img = H / R, n = blockIdx.x / rows_per_img, y0 = (blockIdx.x % rows_per_img) * R;
  // stage the patch: every load first, then split + store
  if constexpr (PL) {
    constexpr int NPR = PH / 2 + 1, NPC = PW / 2 + 1, NIT = NPR * NPC * CIN4, NI = (NIT + NTHR - 1) / NTHR;
    const int Hp = H >> 1, Wp = W >> 1;
    const int iy0 = y0 - pad, ix0 = -pad;        // image row / column of patch pixel (0, 0)
    const int pr0 = iy0 >> 1, pc0 = ix0 >> 1;    // first pooled row / column touching the patch (floor)
    f32x4 v[NI];
    uint32_t aw[NI];
#pragma unroll
    for (int e = 0; e < NI; ++e) {
      const int i = tid + NTHR * e, c4 = i % CIN4, pp = i / CIN4, pr = pr0 + pp / NPC, pc = pc0 + pp % NPC;
      const bool ok = i < NIT && pr >= 0 && pr < Hp && pc >= 0 && pc < Wp;
      const long o = (((long)n * Hp + pr) * Wp + pc) * CIN + 4 * c4;
      v[e] = ok ? *reinterpret_cast<const f32x4*>(dout + o) : f32x4{0.f, 0.f, 0.f, 0.f};
      aw[e] = ok ? *reinterpret_cast<const uint32_t*>(amax + o) : 0u;
    }
#pragma unroll
    for (int e = 0; e < NI; ++e) {
      const int i = tid + NTHR * e;
      if (i < NIT) {
        const int c4 = i % CIN4, pp = i / CIN4, pr = pr0 + pp / NPC, pc = pc0 + pp % NPC;
        sdb::bf16x4 hi, lo;
        sdb::split2(v[e], hi, lo);
        const uint64_t hb = __builtin_bit_cast(uint64_t, hi), lb = __builtin_bit_cast(uint64_t, lo);
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
          const int r = 2 * pr + (qd >> 1) - iy0, c = 2 * pc + (qd & 1) - ix0;
          if ((unsigned)r < (unsigned)PH && (unsigned)c < (unsigned)PW) {
            uint64_t m = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (((aw[e] >> (8 * k)) & 0xffu) == (uint32_t)qd) m |= 0xffffull << (16 * k);
            *reinterpret_cast<uint64_t*>(patch + poff(r * PW + c, 4 * c4)) = hb & m;
            *reinterpret_cast<uint64_t*>(patch + PLANE + poff(r * PW + c, 4 * c4)) = lb & m;
          }
        }
      }
    }
  } else {
    f32x4 v[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int i = tid + NTHR * e, c4 = i % CIN4, pix = i / CIN4, pc = pix % PW, pr = pix / PW;
      const int y = y0 + pr - pad, x = pc - pad;
      v[e] = (i < NEL && y >= 0 && y < H && x >= 0 && x < W)
                 ? *reinterpret_cast<const f32x4*>(dout + (((long)n * H + y) * W + x) * CIN + 4 * c4)
                 : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int i = tid + NTHR * e;
      if (i < NEL) {
        const int c4 = i % CIN4, pix = i / CIN4;
        sdb::bf16x4 hi, lo;
        sdb::split2(v[e], hi, lo);
        *reinterpret_cast<sdb::bf16x4*>(patch + poff(pix, 4 * c4)) = hi;
        *reinterpret_cast<sdb::bf16x4*>(patch + PLANE + poff(pix, 4 * c4)) = lo;
      }
    }
  }
  // this lane's MT pixel tiles: pixel p = 16 MT wave + 16 mt + l16 -> patch-local pixel index (row, x)
  int pbase[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int p = 16 * MT * wave + 16 * mt + l16;
    pbase[mt] = (p >> LW) * PW + (p & (W - 1));
  }
  // B: one k chunk of the pre-split weight ([plane][NOUT][32] bf16, 16-B pieces) per LDS stage, double-buffered and
  // shared by the waves (each wave reading its fragments from global memory itself made the L1 path the bound)
  typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
  constexpr int BROW = 40, SB = 2 * NOUT * BROW, NPC = 8 * NOUT, NPT = (NPC + NTHR - 1) / NTHR;
  __bf16* bst = patch + 2 * PLANE;
  bf16x8 br[NPT];
  auto bload = [&](int kc) {
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int i = tid + NTHR * u;
      if (i < NPC) br[u] = *reinterpret_cast<const bf16x8*>(wsp + (long)(i >> 2) * KP + 32 * kc + 8 * (i & 3));
    }
  };
  auto bstore = [&](int stage) {
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int i = tid + NTHR * u;
      if (i < NPC) *reinterpret_cast<bf16x8*>(bst + stage * SB + (i >> 2) * BROW + 8 * (i & 3)) = br[u];
    }
  };
  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bload(0);
  bstore(0);
  if (NKC > 1) bload(1);
  __syncthreads();
  for (int kc = 0; kc < NKC; ++kc) {
    const __bf16* bs = bst + (kc & 1) * SB + l16 * BROW + 8 * q;
    bf16x8 bh[NT], bl[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      bh[j] = *reinterpret_cast<const bf16x8*>(bs + 16 * j * BROW);
      bl[j] = *reinterpret_cast<const bf16x8*>(bs + (NOUT + 16 * j) * BROW);
    }
    int k0 = 32 * kc + 8 * q;
    k0 = k0 < K ? k0 : K - 8;  // past K: any in-patch address (B is zero there)
    const int tap = k0 / CIN, c0 = k0 - tap * CIN, ky = tap / KS, kx = tap - ky * KS;
    const int toff = ky * PW + kx;
    bf16x8 ah[MT], al[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      ah[mt] = *reinterpret_cast<const bf16x8*>(patch + poff(pbase[mt] + toff, c0));
      al[mt] = *reinterpret_cast<const bf16x8*>(patch + PLANE + poff(pbase[mt] + toff, c0));
    }
    if (kc + 1 < NKC) bstore((kc + 1) & 1);  // chunk kc+1 (loaded one iteration ago) into the other stage
    if (kc + 2 < NKC) bload(kc + 2);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[mt], bh[j], acc[mt][j], 0, 0, 0);
        acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], bl[j], acc[mt][j], 0, 0, 0);
        acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], bh[j], acc[mt][j], 0, 0, 0);
      }
    __syncthreads();
  }
  // acc[mt][j][r]: pixel 16 MT wave + 16 mt + 4 q + r, channel 16 j + l16
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = 16 * MT * wave + 16 * mt + 4 * q + r, y = y0 + (p >> LW), x = p & (W - 1);
      float* o = din + (((long)n * H + y) * W + x) * NOUT + l16;
#pragma unroll
      for (int j = 0; j < NT; ++j) o[16 * j] = acc[mt][j][r];
    }
}

// [plane][n][KP] bf16 split image of a (rows, K) fp32 matrix, KP = K rounded up to 32, zero past K
__global__ __launch_bounds__(256) void split_weight(const float* __restrict__ w, __bf16* __restrict__ out, int rows,
                                                    int K, int KP) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)rows * KP) return;
  const int r = (int)(i / KP), k = (int)(i % KP);
  const float v = k < K ? w[(long)r * K + k] : 0.f;
  const __bf16 hi = (__bf16)v;
  out[i] = hi;
  out[(long)rows * KP + i] = (__bf16)(v - (float)hi);
}

// out[e] = sum_s ws[s * n + e] in a fixed order; 64 outputs per workgroup (one per lane), the 4 waves take every
// 4th slab and are summed through LDS.
// acc.dw set: out is not written; the sums are added into the parameter gradients (element e = (co, j) of the
// (Co, J + 1) [dW | db] layout, J = taps * cx channels; channels >= acc.ci_w dropped)
__global__ __launch_bounds__(256) void slab_reduce(const float* __restrict__ ws, int slabs, long n,
                                                   float* __restrict__ out, sd_wgrad_acc acc, int J, int cx) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long e = (long)blockIdx.x * 64 + lane;
  float v = 0.f;
  if (e < n) {
    int s = wave;
    for (; s + 12 < slabs; s += 16) {
      const float a0 = ws[(long)s * n + e], a1 = ws[(long)(s + 4) * n + e];
      const float a2 = ws[(long)(s + 8) * n + e], a3 = ws[(long)(s + 12) * n + e];
      v += (a0 + a1) + (a2 + a3);
    }
    for (; s < slabs; s += 4) v += ws[(long)s * n + e];
  }
  part[wave][lane] = v;
  __syncthreads();
  if (wave == 0 && e < n) {
    const float r = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    if (!acc.dw) {
      out[e] = r;
    } else {
      const long co = e / (J + 1);
      const int j = (int)(e - co * (J + 1));
      if (j == J) {
        acc.db[co] += r;
      } else {
        const int tap = j / cx, c = j - tap * cx;
        if (c < acc.ci_w) acc.dw[(co * (J / cx) + tap) * acc.ci_w + c] += r;
      }
    }
  }
}

int ilog2_exact(int v) {  // log2(v) if v is a power of two, else -1
  if (v <= 0 || (v & (v - 1))) return -1;
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

template <int BM, int BN, int WM, int WN, bool VA, bool VB>
__global__ __launch_bounds__(256) void conv_fwd_kernel(GemmArgs g, Geom G) {
  const int bn0 = blockIdx.x * BN, bm0 = blockIdx.y * BM;
  Im2colRows<BM, VA> la(G, g.M, bm0);
  DenseOperand<BN, true, VB> lb(g.B, g.ldb, g.N, bn0);
  gemm_block<BM, BN, WM, WN>(g, la, lb, bm0, bn0, 0, 0, 0, g.K);
}

template <int BM, int BN, int WM, int WN, bool VA, bool VB>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(GemmArgs g, Geom G, int J) {
  const int bn0 = blockIdx.x * BN, bm0 = blockIdx.y * BM;
  const int split = blockIdx.z;
  const int kbeg = split * g.kchunk;
  const int kend = min(g.K, kbeg + g.kchunk);
  DenseOperand<BM, false, VA> la(g.A, g.lda, g.M, bm0);
  Im2colCols<BN, VB> lb(G, J, bn0);
  gemm_block<BM, BN, WM, WN>(g, la, lb, bm0, bn0, 0, split, kbeg, kend);
}

// ---------------------------------------------------------------- weight flip, upsample backward
// Wf[ci][ky][kx][co] = W[co][kh-1-ky][kw-1-kx][ci]
__global__ void flip_weight(const float* __restrict__ w, float* __restrict__ wf, int Co, int kh, int kw, int Ci) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)Co * kh * kw * Ci;
  if (t >= total) return;
  const int co = (int)(t % Co);
  long r = t / Co;
  const int kx = (int)(r % kw);
  r /= kw;
  const int ky = (int)(r % kh);
  const int ci = (int)(r / kh);
  wf[t] = w[(((long)co * kh + (kh - 1 - ky)) * kw + (kw - 1 - kx)) * Ci + ci];
}

// dIn[n,Y,X,c] = sum_{dy,dx} dU[n,2Y+dy,2X+dx,c]   (backward of nearest 2x upsample)
__global__ void sumpool2(const float* __restrict__ du, float* __restrict__ din, int Nb, int H, int W, int C) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)Nb * H * W * C;
  if (t >= total) return;
  const int c = (int)(t % C);
  long r = t / C;
  const int X = (int)(r % W);
  r /= W;
  const int Y = (int)(r % H);
  const int n = (int)(r / H);
  const int W2 = 2 * W, H2 = 2 * H;
  const float* b = du + (((long)n * H2 + 2 * Y) * W2 + 2 * X) * C + c;
  din[t] = (b[0] + b[C]) + (b[(long)W2 * C] + b[(long)W2 * C + C]);
}

template <int BM, int BN, int WM, int WN>
void fwd_tile(GemmArgs& g, Geom& G, bool va, bool vb, hipStream_t s) {
  dim3 grid(sd_cdiv(g.N, BN), sd_cdiv(g.M, BM), 1);
  // (the callers' va implies vb)
  with_bools([&](auto VA, auto VB) { conv_fwd_kernel<BM, BN, WM, WN, VA() && VB(), VB()><<<grid, 256, 0, s>>>(g, G); },
             va, vb);
}

template <int BM, int BN, int WM, int WN>
void wgrad_tile(GemmArgs& g, Geom& G, int J, bool va, bool vb, hipStream_t s) {
  dim3 grid(sd_cdiv(g.N, BN), sd_cdiv(g.M, BM), g.ksplit);
  with_bools([&](auto VA, auto VB) { conv_wgrad_kernel<BM, BN, WM, WN, VA(), VB()><<<grid, 256, 0, s>>>(g, G, J); },
             va, vb);
}

// ---------------------------------------------------------------- direct bwd-weight: host plans and launcher
// row-block size, j blocking, split count (shared with the workspace queries) and the staging geometry
struct DirectPlan {
  int R, nbw, gx, gy, slabs;
  bool ws;
  size_t lds;
  int PH, PW, CP, DS;
};
// >= Ci + 2 (the f32 path's ones / zero channels) and, Ci % 4 == 0, >= Ci + 4 (the split-bf16 path's constant quad),
// % 4 == 0, 16 or 48 (mod 64) for wide Ci: the f32 path's word reads are conflict-free, the split-bf16 path's
// transposed reads of its two bf16 planes (the same stride in elements, so half these bytes each) 2-way
int patch_stride(int Ci) {
  if (Ci < 16) return (Ci + 2 + 3) / 4 * 4;
  int c = (Ci + 2 + 15) / 16 * 16;
  while (c % 64 != 16 && c % 64 != 48) c += 16;
  return c;
}
int col_blocks(int kh, int kw, int Ci) { return (kh * kw * Ci + 1 + 15) / 16; }  // 16-column blocks of [dW | db]

// The tail of the four plans, from R, ws, nbw and gx: the staged patch and dy block (x3: the split-bf16 layout), their
// LDS and the grid. False where the staging does not fit.
bool plan_tail(DirectPlan& pl, bool x3, int Nb, int H, int W, int Ci, int Co, int kh, int kw) {
  const int P = pl.R * W;
  pl.PH = pl.R + kh - 1, pl.PW = W + kw - 1, pl.CP = patch_stride(Ci);
  pl.DS = x3 ? P + 8 : Co % 32 == 0 ? Co + 16 : Co;
  const size_t dy_bytes = x3 ? (size_t)((Co + 15) / 16) * 16 * pl.DS * 2 * 2 : (size_t)P * pl.DS * 4;
  pl.lds = (size_t)pl.PH * pl.PW * pl.CP * 4 + dy_bytes;
  if (pl.lds > 160 * 1024 || pl.PH * pl.PW * (Ci / 4) > WD_VP * 512) return false;
  // the wave-split kernel sums its NW_D waves' 16 x 16 tiles through the first NW_D * 4 * 64 floats of LDS at the end:
  // a block that stages less (a 4 x 4 image of 4 channels: 2176 bytes) still gets that much
  if (pl.ws && pl.lds < (size_t)NW_D * 4 * 64 * sizeof(float)) pl.lds = (size_t)NW_D * 4 * 64 * sizeof(float);
  const int blocks = Nb * (H / pl.R);
  pl.gy = 256 / pl.gx;
  if (pl.gy > blocks) pl.gy = blocks;
  if (pl.gy < 1) pl.gy = 1;
  pl.slabs = pl.gy;
  return true;
}

// pixels per staged row block of the max-pool-fused f32 direct bwd-weight (encoder first stage): more pixels per
// block = more MFMA steps per barrier (128 / 256 / 512 px: 397 / 337 / 305 us at 1024 images), falling back to
// smaller blocks where the staging does not fit (pool_plan)
constexpr int WGRAD_POOL_PIX = 512;

// pool_pix > 0: dy arrives at pooled resolution (a quarter of the block's pixels are fetched), blocks of pool_pix px
bool direct_plan(int Nb, int H, int W, int Ci, int Co, int kh, int kw, int ups, DirectPlan& pl, int pool_pix = 0) {
  const bool pool = pool_pix > 0;
  if (ups != 0 || Co % 16 || Co > 64 || Ci % 4 || ilog2_exact(W) < 0) return false;
  const int pix = pool ? pool_pix : 128;
  pl.R = W >= pix ? 1 : (pix / W < H ? pix / W : H);
  if (H % pl.R || (pl.R * W) % 4 || pl.R * W * Co / (pool ? 16 : 4) > WD_VA * 512) return false;
  const int JB = col_blocks(kh, kw, Ci);
  pl.ws = JB <= 7;  // few column blocks: split the pixels over the waves instead
  pl.nbw = pl.ws ? 7 : JB <= 16 ? 2 : JB <= 32 ? 4 : JB <= 56 ? 7 : (Co <= 48 ? 10 : 7);
  pl.gx = pl.ws ? 1 : (JB + NW_D * pl.nbw - 1) / (NW_D * pl.nbw);
  return plan_tail(pl, false, Nb, H, W, Ci, Co, kh, kw);
}

// the pooled plan at the largest block (<= WGRAD_POOL_PIX) whose staging fits
bool pool_plan(int Nb, int H, int W, int Ci, int Co, int kh, int kw, DirectPlan& pl) {
  if (H % 2 || W % 2) return false;
  for (int pix = WGRAD_POOL_PIX; pix >= 128; pix /= 2)
    if (direct_plan(Nb, H, W, Ci, Co, kh, kw, 0, pl, pix) && pl.ws && pl.nbw == 7 && pl.R % 2 == 0) return true;
  return false;
}

// (Ci < 16 is refused: the encoder's 4-channel first stage has its own plan, pool3_plan, or the f32 direct kernel)
bool direct3_plan(int Nb, int H, int W, int Ci, int Co, int kh, int kw, int ups, DirectPlan& pl) {
  if (ups != 0 || Co % 4 || Co > 64 || Ci % 4 || Ci < 16 || W < 8 || ilog2_exact(W) < 0 || W > 128) return false;
  pl.R = 128 / W < H ? 128 / W : H;
  const int P = pl.R * W, JB = col_blocks(kh, kw, Ci);
  if (H % pl.R || P % 32 || (Co / 4) * (P / 4) > 512) return false;
  pl.ws = false;
  // column blocks per wave: the accumulators (TM * NBW * 4 VGPRs) bound it
  const int nmax = Co <= 48 ? 7 : 4;
  pl.gx = (JB + NW_D * nmax - 1) / (NW_D * nmax);
  const int need = (JB + NW_D * pl.gx - 1) / (NW_D * pl.gx);
  pl.nbw = need <= 2 ? 2 : need <= 4 ? 4 : need <= 5 ? 5 : 7;
  return plan_tail(pl, true, Nb, H, W, Ci, Co, kh, kw);
}

// the first stage's plan for conv_wgrad3_direct<TM, 7, WS, PL>: dy at pooled resolution (R even), every wave over
// all <= 7 column blocks (J + 1 <= 112), 32-pixel steps dealt to the 8 waves: R rows of W pixels with 8 steps per
// block (P = 256), one 4-channel x 4-pixel dy item per thread ((Co / 4) (P / 4) <= 512)
bool pool3_plan(int Nb, int H, int W, int Ci, int Co, int kh, int kw, DirectPlan& pl) {
  if (Co % 4 || Co > 64 || Ci % 4 || W < 8 || ilog2_exact(W) < 0 || W > 256 || H % 2) return false;
  if (col_blocks(kh, kw, Ci) > 7) return false;
  pl.R = 256 / W;
  if (pl.R < 2 || pl.R % 2 || H % pl.R || (Co / 4) * (pl.R * W / 4) > 512) return false;
  pl.ws = true;
  pl.nbw = 7;
  pl.gx = 1;
  if (!plan_tail(pl, true, Nb, H, W, Ci, Co, kh, kw)) return false;
  if (Nb < 1) pl.gy = pl.slabs = 0;  // this plan's query answers 0 slabs for no images (the others answer 1)
  return true;
}

// Dynamic LDS above the 64 KiB default has to be granted per kernel: done once, at the kernel's first such launch.
template <auto KERNEL>
bool raise_lds(int bytes) {
  static bool raised = false;
  if (!raised && hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     bytes) != hipSuccess)
    return false;
  return raised = true;
}

// The rungs <TM, NBW, WS, PL> the plans can reach (tests/test_conv_parity_cpu.py enumerates them): 23 of the f32
// kernel, 30 of the split-bf16 one (x3): direct3_plan's 14 in both forms of dy (full resolution, and PL: the pooled
// gradient + argmax of sd_conv2d_wgrad_bf16x3_pooled, the same plan) and pool3_plan's 2. direct3_plan asks for at most
// 4 column blocks per wave at TM 4 and pool3_plan admits Co <= 32, so <4,5>, <4,7>, <3,7,WS,PL> and <4,7,WS,PL> of the
// split-bf16 kernel do not exist.
constexpr bool wd_rung(bool x3, int tm, int nbw, bool ws, bool pl) {
  if (!x3) return ws ? nbw == 7 : !pl && (nbw == 2 || nbw == 4 || nbw == 7 || (nbw == 10 && tm <= 3));
  if (ws) return pl && nbw == 7 && tm <= 2;
  return nbw == 2 || nbw == 4 || (tm <= 3 && (nbw == 5 || nbw == 7));
}
template <bool X3, int TM, int NBW, bool WS, bool PL>
constexpr auto wd_kernel() {
  if constexpr (X3) return &conv_wgrad3_direct<TM, NBW, WS, PL>;
  else return &conv_wgrad_direct<TM, NBW, WS, PL>;
}

// One launch of the plan's rung on the f32 or the split-bf16 (X3) kernel, then the fixed-order sum of its slabs.
// amax set: the pooled-gradient form (PL).
template <bool X3>
int wgrad_direct(const float* in, const float* dout, const uint8_t* amax, float* dw_db, float* ws, long ws_floats,
                 int Nb, int H, int W, int Ci, int Co, int kh, int kw, int pad, const DirectPlan& pl, hipStream_t s,
                 sd_wgrad_acc acc) {
  const int J = kh * kw * Ci;
  const long n = (long)Co * (J + 1);
  if (!ws || ws_floats < pl.slabs * n) return SD_EARG;
  const DirectW d{in, dout, amax, ws, Nb, H, W, Ci, Co, kh, kw, pad, pl.R, ilog2_exact(W),
                  J, pl.PW, pl.PH, pl.CP, pl.DS, Nb * (H / pl.R)};
  int rc = SD_ESHAPE;  // no such rung
  with_int<1, 2, 3, 4>((Co + 15) / 16, [&](auto TM) {
    with_int<2, 4, 5, 7, 10>(pl.nbw, [&](auto NBW) {
      with_bools(
          [&](auto WS, auto PL) {
            constexpr int tm = decltype(TM)::value, nbw = decltype(NBW)::value;
            constexpr bool wsplit = decltype(WS)::value, pooled = decltype(PL)::value;
            if constexpr (wd_rung(X3, tm, nbw, wsplit, pooled)) {
              constexpr auto kernel = wd_kernel<X3, tm, nbw, wsplit, pooled>();
              rc = pl.lds > 65536 && !raise_lds<kernel>(160 * 1024) ? SD_EARG : SD_OK;
              if (rc == SD_OK) kernel<<<dim3(pl.gx, pl.gy), 512, pl.lds, s>>>(d);
            }
          },
          pl.ws, amax != nullptr);
    });
  });
  if (rc != SD_OK) return rc;
  SD_LAUNCH_CHECK();
  slab_reduce<<<(int)((n + 63) / 64), 256, 0, s>>>(ws, pl.slabs, n, dw_db, acc, J, Ci);  // 4 waves x unrolled loads
  SD_LAUNCH_CHECK();
  return SD_OK;
}

// the optional parameter-gradient target of the bwd-weight entries; false for an inconsistent one
bool wgrad_acc_arg(const sd_wgrad_acc* acc_p, int Ci, sd_wgrad_acc& acc) {
  acc = acc_p ? *acc_p : sd_wgrad_acc{nullptr, nullptr, 0};
  return !acc.dw || (acc.db && acc.ci_w >= 1 && acc.ci_w <= Ci);
}
}  // namespace

// out (Nb, Hg, Wg, Co) = conv_same(in (Nb, Hs, Ws, Ci) [upsampled x2 if ups], w (Co, kh, kw, Ci)) + bias
extern "C" int sd_conv2d_fwd(const float* in, const float* w, const float* bias, float* out, int Nb, int Hs, int Ws,
                             int Ci, int Co, int kh, int kw, int pad, int ups, sd_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (Nb <= 0) return SD_OK;
  Geom G{in, Nb, Hs, Ws, Ci, Hs << ups, Ws << ups, kh, kw, pad, ups};
  GemmArgs g{};
  g.B = w; g.C = out; g.bias = bias; g.ldb = (long)kh * kw * Ci; g.ldc = Co;
  g.M = Nb * G.Hg * G.Wg; g.N = Co; g.K = kh * kw * Ci; g.batch = 1; g.ksplit = 1; g.kchunk = g.K;
  g.alpha = 1.f; g.beta = 0.f;
  const bool vb = (((long)kh * kw * Ci) % 4 == 0) && aligned16(w);
  const bool va = (Ci % 4 == 0) && aligned16(in) && vb;
  const int lw = ilog2_exact(G.Wg), lhw = ilog2_exact(G.Hg * G.Wg);
  if (va && lw >= 0 && lhw >= 0 && g.K / 4 <= MAX_TAPQ && (Co == 32 || Co == 48 || Co == 64 || Co == 16)) {
    const dim3 grid(sd_cdiv(g.M, 128));
    // the early-store main loop with buffer-load operands while every buffer offset is < 2 GiB, else the
    // double-buffered main loop with branchy loaders
    const bool es = (long)Nb * Hs * Ws * Ci < (1L << 29);
#define SD_FWD16(BN) (es ? conv_fwd16<BN, true><<<grid, 256, 0, s>>>(g, G, lw, lhw) \
                         : conv_fwd16<BN, false><<<grid, 256, 0, s>>>(g, G, lw, lhw))
    switch (Co) {
      case 16: SD_FWD16(16); break;
      case 32: SD_FWD16(32); break;
      case 48: SD_FWD16(48); break;
      default: SD_FWD16(64); break;
    }
#undef SD_FWD16
  } else if (Co <= 32) fwd_tile<128, 32, 32, 32>(g, G, va, vb, s);
  else fwd_tile<128, 64, 64, 32>(g, G, va, vb, s);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

// dw_db (Co, kh*kw*Ci + 1) = [dW | d bias] = sum over pixels of dout (Nb,Hg,Wg,Co) x im2col(in)
// fused ConvEncoder stage forward; SD_ESHAPE when the shape is outside the fused kernel (caller: conv + pool)
template <class NW>
static int fwd_pool_impl(const float* in, const float* w, const float* bias, NW nw, float* pooled, uint8_t* amax,
                         float* y, float* rstd, int Nb, int Hs, int Ws, int Ci, int Co, int kh, int kw, int pad,
                         float eps, int nchw_flat, sd_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (Nb <= 0) return SD_OK;
  Geom G{in, Nb, Hs, Ws, Ci, Hs, Ws, kh, kw, pad, 0};
  GemmArgs g{};
  g.B = w; g.bias = bias; g.ldb = (long)kh * kw * Ci; g.ldc = Co;
  g.M = Nb * Hs * Ws; g.N = Co; g.K = kh * kw * Ci; g.batch = 1; g.ksplit = 1; g.kchunk = g.K;
  g.alpha = 1.f; g.beta = 0.f;
  const bool vb = (((long)kh * kw * Ci) % 4 == 0) && aligned16(w);
  const bool va = (Ci % 4 == 0) && aligned16(in) && vb;
  const int lw = ilog2_exact(Ws), lhw = ilog2_exact(Hs * Ws);
  if (!va || lw < 1 || lhw < 0 || g.K / 4 > MAX_TAPQ || Hs % 2 || 128 % (2 * Ws) || g.M % 128) return SD_ESHAPE;
  const dim3 grid(g.M / 128);
  const bool es = (long)Nb * Hs * Ws * Ci < (1L << 29);  // buffer offsets < 2 GiB
  if (es && Co == 48 && Ci == 32 && Ws == 32 && kh == 5 && kw == 5 && pad == 2 && Hs % 4 == 0 && aligned16(in)) {
    conv_fwd_direct_pool<48, 32, 5, 5, NW><<<g.M / 128, 256, 0, s>>>(g, G, lhw, nw, pooled, amax, y, rstd, eps,
                                                                     nchw_flat);
    SD_LAUNCH_CHECK();
    return SD_OK;
  }
  if (es && Co == 32 && Ci == 4 && Ws == 64 && kh == 5 && kw == 5 && pad == 2 && Hs % 2 == 0 && aligned16(in)) {
    // one round of resident workgroups (4 per CU): tpw tiles each. (The round-5 grid was 16 tiles per workgroup: 2048
    // workgroups at 1024 images, 2.67 rounds of the 768 then resident.)
    const int tiles = g.M / 128, tpw = sd_cdiv(tiles, 1024), nwg = sd_cdiv(tiles, tpw);
    conv_fwd_direct_pool_c4<32, 6, 5, 4, NW><<<nwg, 256, 0, s>>>(g, G, lhw, tpw, nw, pooled, amax, y, rstd, eps,
                                                                 nchw_flat);
    SD_LAUNCH_CHECK();
    return SD_OK;
  }
#define SD_FWDP(BN)                                                                                              \
  (es ? conv_fwd16_pool<BN, true, NW><<<grid, 256, 0, s>>>(g, G, lw, lhw, nw, pooled, amax, y, rstd, eps, nchw_flat) \
      : conv_fwd16_pool<BN, false, NW><<<grid, 256, 0, s>>>(g, G, lw, lhw, nw, pooled, amax, y, rstd, eps, nchw_flat))
  switch (Co) {
    case 16: SD_FWDP(16); break;
    case 32: SD_FWDP(32); break;
    case 48: SD_FWDP(48); break;
    case 64: SD_FWDP(64); break;
    default: return SD_ESHAPE;
  }
#undef SD_FWDP
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_conv2d_fwd_pool(const float* in, const float* w, const float* bias, const float* nw, float* pooled,
                                  uint8_t* amax, float* y, float* rstd, int Nb, int Hs, int Ws, int Ci, int Co, int kh,
                                  int kw, int pad, float eps, int nchw_flat, sd_stream stream_) {
  return fwd_pool_impl(in, w, bias, nw, pooled, amax, y, rstd, Nb, Hs, Ws, Ci, Co, kh, kw, pad, eps, nchw_flat,
                       stream_);
}

// the FiLM stage on the same kernels: gamma / beta (Nb / ipc, Co), ipc images per context row
extern "C" int sd_conv2d_fwd_pool_film(const float* in, const float* w, const float* bias, const float* nw,
                                       const float* gamma, const float* beta, int ipc, float* pooled, uint8_t* amax,
                                       float* y, float* rstd, int Nb, int Hs, int Ws, int Ci, int Co, int kh, int kw,
                                       int pad, float eps, int nchw_flat, sd_stream stream_) {
  if (!gamma || !beta || ipc <= 0 || Nb % ipc) return SD_EARG;
  return fwd_pool_impl(in, w, bias, FilmNW{nw, gamma, beta, ipc}, pooled, amax, y, rstd, Nb, Hs, Ws, Ci, Co, kh, kw,
                       pad, eps, nchw_flat, stream_);
}

extern "C" int sd_conv2d_wgrad(const float* in, const float* dout, float* dw_db, float* workspace, long ws_floats,
                               int ksplit, int Nb, int Hs, int Ws, int Ci, int Co, int kh, int kw, int pad, int ups,
                               const sd_wgrad_acc* acc_p, sd_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (Nb <= 0) return SD_OK;
  sd_wgrad_acc acc;
  if (!wgrad_acc_arg(acc_p, Ci, acc) || (acc.dw && !dw_db)) return SD_EARG;
  Geom G{in, Nb, Hs, Ws, Ci, Hs << ups, Ws << ups, kh, kw, pad, ups};
  const int J = kh * kw * Ci;
  GemmArgs g{};
  g.A = dout; g.lda = Co; g.C = dw_db; g.ldc = J + 1; g.ws = workspace;
  g.M = Co; g.N = J + 1; g.K = Nb * G.Hg * G.Wg; g.batch = 1;
  int ks = ksplit < 1 ? 1 : ksplit;
  if (ks > 1 && (!workspace || ws_floats < (long)ks * g.M * g.N)) return SD_EARG;
  g.ksplit = ks;
  long kc = ((long)g.K + ks - 1) / ks;
  g.kchunk = (int)((kc + BK - 1) / BK * BK);
  g.alpha = 1.f; g.beta = 0.f;
  const bool va = aligned16(dout) && Co % 4 == 0;
  const bool vb = (Ci % 4 == 0) && aligned16(in);
  DirectPlan pl;
  if (va && vb && direct_plan(Nb, Hs, Ws, Ci, Co, kh, kw, ups, pl))
    return wgrad_direct<false>(in, dout, nullptr, dw_db, workspace, ws_floats, Nb, Hs, Ws, Ci, Co, kh, kw, pad, pl,
                               s, acc);
  if (Co <= 32) wgrad_tile<32, 128, 32, 32>(g, G, J, va, vb, s);
  else wgrad_tile<64, 64, 32, 32>(g, G, J, va, vb, s);
  SD_LAUNCH_CHECK();
  if (ks > 1) {
    launch_reduce(g, s, false);
    SD_LAUNCH_CHECK();
  }
  if (acc.dw) {  // the implicit-GEMM path wrote dw_db: one pass adds it into the gradients
    const long total = (long)Co * (J + 1);
    slab_reduce<<<(int)((total + 63) / 64), 256, 0, s>>>(dw_db, 1, total, nullptr, acc, J, Ci);
    SD_LAUNCH_CHECK();
  }
  return SD_OK;
}

// number of partial slabs (each Co x (kh*kw*Ci+1) floats) sd_conv2d_wgrad will use with this `ksplit` request
extern "C" int sd_conv2d_wgrad_slabs(int Nb, int Hs, int Ws, int Ci, int Co, int kh, int kw, int ups, int ksplit) {
  DirectPlan pl;
  if (direct_plan(Nb, Hs, Ws, Ci, Co, kh, kw, ups, pl)) return pl.slabs;
  return ksplit < 1 ? 1 : ksplit;
}

// bwd-weight of a pooled stage straight from the max-pool backward's pooled-resolution gradient + argmax
// (sd_pool_rms_bwd_compact, poolnorm.hip): the direct f32 kernel expands it while staging. SD_ESHAPE outside the
// direct plan.
extern "C" int sd_conv2d_wgrad_pool_slabs(int Nb, int H, int W, int Ci, int Co, int kh, int kw) {
  DirectPlan pl;
  if (!pool_plan(Nb, H, W, Ci, Co, kh, kw, pl)) return 0;
  return pl.slabs;
}
extern "C" int sd_conv2d_wgrad_pool(const float* in, const float* dpool, const uint8_t* amax, float* dw_db,
                                    float* workspace, long ws_floats, int Nb, int H, int W, int Ci, int Co, int kh,
                                    int kw, int pad, const sd_wgrad_acc* acc_p, sd_stream stream_) {
  if (Nb <= 0) return SD_OK;
  sd_wgrad_acc acc;
  if (!wgrad_acc_arg(acc_p, Ci, acc)) return SD_EARG;
  DirectPlan pl;
  if (!pool_plan(Nb, H, W, Ci, Co, kh, kw, pl))
    return SD_ESHAPE;
  // amax is read as uint32 words (4 pooled pixels' argmax bytes per load)
  if (!aligned16(dpool) || !aligned16(in) || Co % 4 || Ci % 4 || !amax || reinterpret_cast<uintptr_t>(amax) % 4)
    return SD_EARG;
  return wgrad_direct<false>(in, dpool, amax, dw_db, workspace, ws_floats, Nb, H, W, Ci, Co, kh, kw, pad, pl,
                             (hipStream_t)stream_, acc);
}

extern "C" int sd_conv_flip_weight(const float* w, float* wf, int Co, int kh, int kw, int Ci, sd_stream s) {
  const long total = (long)Co * kh * kw * Ci;
  flip_weight<<<(int)((total + 255) / 256), 256, 0, (hipStream_t)s>>>(w, wf, Co, kh, kw, Ci);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_sumpool2(const float* du, float* din, int Nb, int H, int W, int C, sd_stream s) {
  const long total = (long)Nb * H * W * C;
  if (total <= 0) return SD_OK;
  sumpool2<<<(int)((total + 255) / 256), 256, 0, (hipStream_t)s>>>(du, din, Nb, H, W, C);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_conv2d_dgrad_bf16x3(const float* dout, const float* wflip, float* din, int Nb, int Hs, int Ws,
                                      int Ci, int Co, int kh, int kw, int pad, sd_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (Nb <= 0) return SD_OK;
  Geom G{dout, Nb, Hs, Ws, Ci, Hs, Ws, kh, kw, pad, 0};
  GemmArgs g{};
  g.B = wflip; g.C = din; g.ldb = (long)kh * kw * Ci; g.ldc = Co;
  g.M = Nb * Hs * Ws; g.N = Co; g.K = kh * kw * Ci; g.batch = 1; g.ksplit = 1; g.kchunk = g.K;
  g.alpha = 1.f; g.beta = 0.f;
  const int lw = ilog2_exact(Ws), lhw = ilog2_exact(Hs * Ws);
  if (Ci % 4 || !aligned16(dout) || !aligned16(wflip) || lw < 0 || lhw < 0 || g.K / 4 > MAX_TAPQ ||
      (long)Nb * Hs * Ws * Ci >= (1L << 29))
    return SD_ESHAPE;
  const dim3 grid(sd_cdiv(g.M, 128));
  switch (Co) {
    case 16: conv_dgrad3<16><<<grid, 256, 0, s>>>(g, G, lw, lhw); break;
    case 32: conv_dgrad3<32><<<grid, 256, 0, s>>>(g, G, lw, lhw); break;
    case 48: conv_dgrad3<48><<<grid, 256, 0, s>>>(g, G, lw, lhw); break;
    case 64: conv_dgrad3<64><<<grid, 256, 0, s>>>(g, G, lw, lhw); break;
    default: return SD_ESHAPE;
  }
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_conv_split3_weight(const float* w, void* wsplit, int rows, int K, sd_stream stream_) {
  if (rows <= 0 || K <= 0 || !w || !wsplit) return SD_EARG;
  const int KP = (K + 31) / 32 * 32;
  const long total = (long)rows * KP;
  split3_weight<<<(int)((total + 255) / 256), 256, 0, (hipStream_t)stream_>>>(w, static_cast<__bf16*>(wsplit), rows,
                                                                               K, KP);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

namespace {
// SDHIP_CONV6_RING=0: the per-lane-weight kernel (conv_fwd6_direct_pool) instead of the LDS-ring one. Not an A/B
// switch: the per-lane kernel is the simple form of the algorithm and the bit-exact oracle of the ring kernel's test.
bool conv6_ring() {  // read per call (host only): the test toggles it in-process
  const char* e = getenv("SDHIP_CONV6_RING");
  return e ? atoi(e) != 0 : true;
}
template <int BN, int CI, int LW, int KS, int TPW, int MT, int BROW, class NW>
int fwd6r_launch_t(const GemmArgs& g, const Geom& G, int lhw, const __bf16* wsp, NW nw, float* pooled,
                   uint8_t* amax, float* y, float* rstd, float eps, int nchw_flat, hipStream_t s) {
  // the channel-group-major patch (three planes, MT * 128 pixels + halo) and the ring
  constexpr int W = 1 << LW, R = MT * 128 / W;
  constexpr size_t lds = (size_t)3 * (R + KS - 1) * (W + KS - 1) * CI * 2 + (size_t)2 * 3 * BN * BROW * 2;
  static_assert(lds <= 160 * 1024, "LDS");
  if (!raise_lds<&conv_fwd6r_direct_pool<BN, CI, LW, KS, TPW, MT, BROW, NW>>((int)lds)) return SD_EARG;
  const int nwg = (sd_cdiv(g.M / (MT * 128), TPW) + 7) / 8 * 8;  // a multiple of 8: XCD-contiguous
  conv_fwd6r_direct_pool<BN, CI, LW, KS, TPW, MT, BROW, NW><<<nwg, 512, lds, s>>>(g, G, lhw, wsp, nw, pooled, amax, y,
                                                                                  rstd, eps, nchw_flat);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
// The two shapes sd_conv2d_fwd_pool6 accepts (square images: every tile below is whole rows of one image).
// 32 -> 48 at 32 x 32: 512-pixel tiles, 64 pixels per wave, packed ring (356 vs 392 us alone against the 256-pixel
// tiles of 32-pixel waves with a padded pixel-major patch, profiles/r06mt4), one tile per workgroup: with more, its
// prefetch registers spilled (386 us).
// 48 -> 64 at 16 x 16: whole-image 256-pixel tiles, padded ring, enough tiles per workgroup (1, 2, 4, 8, 16) for one
// workgroup per CU.
template <int BN, int CI, int LW, class NW>
int fwd6_launch(const GemmArgs& g, const Geom& G, int lhw, const __bf16* wsp, NW nw, float* pooled,
                uint8_t* amax, float* y, float* rstd, float eps, int nchw_flat, hipStream_t s) {
  constexpr int W = 1 << LW, R = 128 / W, KS = 5;
  static_assert((BN == 48 && CI == 32 && LW == 5) || (BN == 64 && CI == 48 && LW == 4), "the two encoder stages");
  if (conv6_ring()) {
#define SD_F6R(T, MT, BROW) \
  fwd6r_launch_t<BN, CI, LW, KS, T, MT, BROW>(g, G, lhw, wsp, nw, pooled, amax, y, rstd, eps, nchw_flat, s)
    if constexpr (CI == 32) {
      return SD_F6R(1, 4, 32);
    } else {
      const int want = sd_cdiv(g.M / 256, 256);
      return want <= 1 ? SD_F6R(1, 2, 40) : want <= 2 ? SD_F6R(2, 2, 40) : want <= 4 ? SD_F6R(4, 2, 40)
           : want <= 8 ? SD_F6R(8, 2, 40) : SD_F6R(16, 2, 40);
    }
#undef SD_F6R
  }
  const size_t lds = (size_t)3 * (R + KS - 1) * (W + KS - 1) * (CI + 8) * 2;
  if (lds > 65536 && !raise_lds<&conv_fwd6_direct_pool<BN, CI, LW, KS, NW>>((int)lds)) return SD_EARG;
  conv_fwd6_direct_pool<BN, CI, LW, KS, NW><<<g.M / 128, 256, lds, s>>>(g, G, lhw, wsp, nw, pooled, amax, y, rstd, eps,
                                                                   nchw_flat);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
}  // namespace

template <class NW>
static int fwd_pool6_impl(const float* in, const void* wsplit3, const float* bias, NW nw, float* pooled, uint8_t* amax,
                          float* y, float* rstd, int Nb, int Hs, int Ws, int Ci, int Co, int kh, int kw, int pad,
                          float eps, int nchw_flat, sd_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (Nb <= 0) return SD_OK;
  if (kh != 5 || kw != 5 || pad != 2 || Hs != Ws || Hs % 2 || !aligned16(in) || !aligned16(wsplit3)) return SD_ESHAPE;
  Geom G{in, Nb, Hs, Ws, Ci, Hs, Ws, kh, kw, pad, 0};
  GemmArgs g{};
  g.bias = bias; g.M = Nb * Hs * Ws; g.N = Co; g.K = kh * kw * Ci;
  const int lhw = ilog2_exact(Hs * Ws);
  if (lhw < 0 || g.M % 128) return SD_ESHAPE;
  const __bf16* wsp = static_cast<const __bf16*>(wsplit3);
  // a 128-pixel tile is 128 / Ws whole rows of one image
  if (Co == 48 && Ci == 32 && Ws == 32)
    return fwd6_launch<48, 32, 5>(g, G, lhw, wsp, nw, pooled, amax, y, rstd, eps, nchw_flat, s);
  if (Co == 64 && Ci == 48 && Ws == 16)
    return fwd6_launch<64, 48, 4>(g, G, lhw, wsp, nw, pooled, amax, y, rstd, eps, nchw_flat, s);
  return SD_ESHAPE;
}

extern "C" int sd_conv2d_fwd_pool6(const float* in, const void* wsplit3, const float* bias, const float* nw,
                                   float* pooled, uint8_t* amax, float* y, float* rstd, int Nb, int Hs, int Ws, int Ci,
                                   int Co, int kh, int kw, int pad, float eps, int nchw_flat, sd_stream stream_) {
  return fwd_pool6_impl(in, wsplit3, bias, nw, pooled, amax, y, rstd, Nb, Hs, Ws, Ci, Co, kh, kw, pad, eps, nchw_flat,
                        stream_);
}

extern "C" int sd_conv2d_fwd_pool6_film(const float* in, const void* wsplit3, const float* bias, const float* nw,
                                        const float* gamma, const float* beta, int ipc, float* pooled, uint8_t* amax,
                                        float* y, float* rstd, int Nb, int Hs, int Ws, int Ci, int Co, int kh, int kw,
                                        int pad, float eps, int nchw_flat, sd_stream stream_) {
  if (!gamma || !beta || ipc <= 0 || Nb % ipc) return SD_EARG;
  return fwd_pool6_impl(in, wsplit3, bias, FilmNW{nw, gamma, beta, ipc}, pooled, amax, y, rstd, Nb, Hs, Ws, Ci, Co,
                        kh, kw, pad, eps, nchw_flat, stream_);
}

extern "C" int sd_conv_split_weight(const float* w, void* wsplit, int rows, int K, sd_stream stream_) {
  if (rows <= 0 || K <= 0 || !w || !wsplit) return SD_EARG;
  const int KP = (K + 31) / 32 * 32;
  const long total = (long)rows * KP;
  split_weight<<<(int)((total + 255) / 256), 256, 0, (hipStream_t)stream_>>>(w, static_cast<__bf16*>(wsplit), rows, K,
                                                                              KP);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

namespace {
// R whole image rows per workgroup as NTHR / 64 waves of 64 pixels, channel-group-major patch
// amax set: dout is the pooled-resolution gradient (PL)
template <int CIN, int NT, int LW, int R, int NTHR, bool PL>
int dgrad_direct_launch(const float* dout, const uint8_t* amax, const __bf16* wsp, float* din, int Nb, int H, int pad,
                        hipStream_t s) {
  constexpr int W = 1 << LW, KS = 5;
  static_assert(R * W == NTHR, "64-pixel waves");
  constexpr size_t lds = (size_t)2 * (R + KS - 1) * (W + KS - 1) * CIN * 2 + (size_t)2 * 2 * (16 * NT) * 40 * 2;
  static_assert(lds <= 160 * 1024, "LDS");
  if (H % R) return SD_ESHAPE;
  if (!raise_lds<&conv_dgrad3_direct<CIN, NT, LW, KS, NTHR, PL>>((int)lds)) return SD_EARG;
  conv_dgrad3_direct<CIN, NT, LW, KS, NTHR, PL><<<Nb * (H / R), NTHR, lds, s>>>(dout, amax, wsp, din, Nb, H, pad);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
// the two shapes of the direct bwd-data kernel (Ci = dOut's channels, Co = dIn's): 1 = 48 -> 32 at 32 x 32 images as
// 512-pixel tiles (16 rows) over 8 waves, one workgroup per CU; 2 = 64 -> 48 at 16 x 16 as whole-image 256-pixel tiles
// over 4 waves (183 -> 131 us alone against 128-pixel tiles of 32-pixel waves, profiles/r06dg3); 0 = neither
int dgrad_direct_shape(int Hs, int Ws, int Ci, int Co, int kh, int kw, int pad) {
  if (kh != 5 || kw != 5 || pad != 2 || Hs != Ws) return 0;
  return Ci == 48 && Co == 32 && Ws == 32 ? 1 : Ci == 64 && Co == 48 && Ws == 16 ? 2 : 0;
}
template <bool PL>
int dgrad_direct(const float* dout, const uint8_t* amax, const void* wsplit, float* din, int Nb, int Hs, int Ws, int Ci,
                 int Co, int kh, int kw, int pad, hipStream_t s) {
  const __bf16* wsp = static_cast<const __bf16*>(wsplit);
  switch (dgrad_direct_shape(Hs, Ws, Ci, Co, kh, kw, pad)) {
    case 1: return dgrad_direct_launch<48, 2, 5, 16, 512, PL>(dout, amax, wsp, din, Nb, Hs, pad, s);
    case 2: return dgrad_direct_launch<64, 3, 4, 16, 256, PL>(dout, amax, wsp, din, Nb, Hs, pad, s);
    default: return SD_ESHAPE;
  }
}
}  // namespace

extern "C" int sd_conv2d_dgrad_direct(const float* dout, const void* wsplit, float* din, int Nb, int Hs, int Ws,
                                      int Ci, int Co, int kh, int kw, int pad, sd_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (Nb <= 0) return SD_OK;
  if (kh != 5 || kw != 5 || pad != 2 || Hs != Ws || !aligned16(dout) || !aligned16(wsplit) || !aligned16(din))
    return SD_ESHAPE;
  return dgrad_direct<false>(dout, nullptr, wsplit, din, Nb, Hs, Ws, Ci, Co, kh, kw, pad, s);
}

// sd_conv2d_dgrad_direct of a pooled stage from (dpool, argmax): din (Nb, Hs, Ws, Co) = that entry's on
// expand(dpool, amax), bit for bit, for the same two shapes (Hs, Ws: the full resolution; dpool and amax are
// (Nb, Hs / 2, Ws / 2, Ci)). _ok: 1 where the shape is taken.
extern "C" int sd_conv2d_dgrad_direct_pooled_ok(int Hs, int Ws, int Ci, int Co, int kh, int kw, int pad) {
  return dgrad_direct_shape(Hs, Ws, Ci, Co, kh, kw, pad) != 0;
}
extern "C" int sd_conv2d_dgrad_direct_pooled(const float* dpool, const uint8_t* amax, const void* wsplit, float* din,
                                             int Nb, int Hs, int Ws, int Ci, int Co, int kh, int kw, int pad,
                                             sd_stream stream_) {
  if (!sd_conv2d_dgrad_direct_pooled_ok(Hs, Ws, Ci, Co, kh, kw, pad)) return SD_ESHAPE;
  if (Nb <= 0) return SD_OK;
  // amax is read as uint32 words (4 channels' argmax bytes per load)
  if (!dpool || !amax || !wsplit || !din || !aligned16(dpool) || !aligned16(wsplit) || !aligned16(din) ||
      reinterpret_cast<uintptr_t>(amax) % 4)
    return SD_EARG;
  return dgrad_direct<true>(dpool, amax, wsplit, din, Nb, Hs, Ws, Ci, Co, kh, kw, pad, (hipStream_t)stream_);
}

extern "C" int sd_conv2d_wgrad_bf16x3_slabs(int Nb, int Hs, int Ws, int Ci, int Co, int kh, int kw, int ups) {
  DirectPlan pl;
  if (!direct3_plan(Nb, Hs, Ws, Ci, Co, kh, kw, ups, pl)) return SD_ESHAPE;
  return pl.slabs;
}

extern "C" int sd_conv2d_wgrad_pool_bf16x3_slabs(int Nb, int H, int W, int Ci, int Co, int kh, int kw) {
  DirectPlan pl;
  if (!pool3_plan(Nb, H, W, Ci, Co, kh, kw, pl)) return 0;
  return pl.slabs;
}
extern "C" int sd_conv2d_wgrad_pool_bf16x3(const float* in, const float* dpool, const uint8_t* amax, float* dw_db,
                                           float* workspace, long ws_floats, int Nb, int H, int W, int Ci, int Co,
                                           int kh, int kw, int pad, const sd_wgrad_acc* acc_p, sd_stream stream_) {
  if (Nb <= 0) return SD_OK;
  sd_wgrad_acc acc;
  if (!wgrad_acc_arg(acc_p, Ci, acc)) return SD_EARG;
  DirectPlan pl;
  if (!pool3_plan(Nb, H, W, Ci, Co, kh, kw, pl)) return SD_ESHAPE;
  if (!aligned16(dpool) || !aligned16(in) || !amax || reinterpret_cast<uintptr_t>(amax) % 4) return SD_EARG;
  return wgrad_direct<true>(in, dpool, amax, dw_db, workspace, ws_floats, Nb, H, W, Ci, Co, kh, kw, pad, pl,
                            (hipStream_t)stream_, acc);
}

extern "C" int sd_conv2d_wgrad_bf16x3(const float* in, const float* dout, float* dw_db, float* workspace,
                                      long ws_floats, int Nb, int Hs, int Ws, int Ci, int Co, int kh, int kw, int pad,
                                      const sd_wgrad_acc* acc_p, sd_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (Nb <= 0) return SD_OK;
  sd_wgrad_acc acc;
  if (!wgrad_acc_arg(acc_p, Ci, acc)) return SD_EARG;
  DirectPlan pl;
  if (!direct3_plan(Nb, Hs, Ws, Ci, Co, kh, kw, 0, pl) || !aligned16(in) || !aligned16(dout)) return SD_ESHAPE;
  return wgrad_direct<true>(in, dout, nullptr, dw_db, workspace, ws_floats, Nb, Hs, Ws, Ci, Co, kh, kw, pad, pl,
                            s, acc);
}

// sd_conv2d_wgrad_bf16x3 of a pooled stage from (dpool, argmax): direct3_plan's own plan (the same rung, R, gx and
// slabs as on the full-resolution gradient) with dy expanded while it is staged, so the same values reach the same LDS
// slots and [dW | db] is that entry's on expand(dpool, amax) bit for bit. H even on top of the plan (W is a power of
// two >= 8); the query answers 0 outside it.
extern "C" int sd_conv2d_wgrad_bf16x3_pooled_slabs(int Nb, int H, int W, int Ci, int Co, int kh, int kw) {
  DirectPlan pl;
  if (H % 2 || !direct3_plan(Nb, H, W, Ci, Co, kh, kw, 0, pl)) return 0;
  return pl.slabs;
}
extern "C" int sd_conv2d_wgrad_bf16x3_pooled(const float* in, const float* dpool, const uint8_t* amax, float* dw_db,
                                             float* workspace, long ws_floats, int Nb, int H, int W, int Ci, int Co,
                                             int kh, int kw, int pad, const sd_wgrad_acc* acc_p, sd_stream stream_) {
  if (Nb <= 0) return SD_OK;
  sd_wgrad_acc acc;
  if (!wgrad_acc_arg(acc_p, Ci, acc)) return SD_EARG;
  DirectPlan pl;
  if (H % 2 || !direct3_plan(Nb, H, W, Ci, Co, kh, kw, 0, pl)) return SD_ESHAPE;
  if (!aligned16(dpool) || !aligned16(in) || !amax || reinterpret_cast<uintptr_t>(amax) % 4) return SD_EARG;
  return wgrad_direct<true>(in, dpool, amax, dw_db, workspace, ws_floats, Nb, H, W, Ci, Co, kh, kw, pad, pl,
                            (hipStream_t)stream_, acc);
}

// ---------------------------------------------------------------- first-stage input gradient from the pooled gradient
// dIn (Nb, H, 64, 3) = conv_same(expand(dpool, amax), flipped W) for the encoder's first stage (32 -> 3 channels, 5x5,
// pad 2). A workgroup owns a 16-row x 64-column tile of one image; the conv gradient of that tile (+ 2 halo rows /
// columns) exists only in LDS, 8 output channels at a time: each of the 10 x 32 pooled pixels of the slab writes its
// gradient at the argmax position of its 2x2 window and zeros at the other three. A thread owns one column and four
// rows (12 f32 accumulators); per (kx, 4 channels) it reads 8 rows as float4 (column stride 12 floats: the 16 lanes of
// a ds_read_b128 phase hit 16 distinct bank quads) and issues 240 FMAs whose weight operand is wave-uniform (scalar
// loads of w). Plain f32 FMAs in a fixed (channel chunk, kx, channel, row, ky) order: no atomics, no split products.
namespace {
constexpr int DP_CO = 32, DP_KS = 5, DP_W = 64, DP_CI = 3, DP_TH = 16, DP_R = 4, DP_CC = 8, DP_CS = 12;
constexpr int DP_LW = DP_W + DP_KS - 1, DP_LR = DP_TH + DP_KS - 1, DP_RS = DP_LW * DP_CS;

__global__ __launch_bounds__(256, 2) void conv_dgrad_pool_k(const float* __restrict__ dpool,
                                                           const uint8_t* __restrict__ amax,
                                                           const float* __restrict__ w, float* __restrict__ din,
                                                           int H) {
  __shared__ __attribute__((aligned(16))) float tile[DP_LR * DP_RS];
  const int tid = threadIdx.x;
  const int tiles = (H + DP_TH - 1) / DP_TH;
  const int n = blockIdx.x / tiles, y0 = (blockIdx.x % tiles) * DP_TH;
  const int Ho = H / 2, Wo = DP_W / 2;
  // halo columns (outside the image) stay zero for every channel chunk
  for (int i = tid; i < DP_LR * 4 * DP_CC; i += 256) {
    const int c = i % DP_CC, h = (i / DP_CC) % 4, r = i / (4 * DP_CC);
    tile[r * DP_RS + (h < 2 ? h : DP_W + h) * DP_CS + c] = 0.f;
  }
  const int sx = tid / DP_CC, sc = tid % DP_CC;  // staging: pooled column, channel of the chunk
  const int x = tid % DP_W, l0 = (tid / DP_W) * DP_R;
  float acc[DP_R][DP_CI];
#pragma unroll
  for (int r = 0; r < DP_R; ++r)
#pragma unroll
    for (int ci = 0; ci < DP_CI; ++ci) acc[r][ci] = 0.f;

  for (int c0 = 0; c0 < DP_CO; c0 += DP_CC) {
    if (c0) __syncthreads();
    // pooled rows y0/2 - 1 .. y0/2 + 8 -> conv-gradient rows y0 - 2 .. y0 + 17 (tile rows 0 .. 19)
    for (int i = 0; i < DP_LR / 2; ++i) {
      const int pr = y0 / 2 - 1 + i;
      float dp = 0.f;
      int q = 0;
      if (pr >= 0 && pr < Ho) {
        const long o = (((long)n * Ho + pr) * Wo + sx) * DP_CO + c0 + sc;
        dp = dpool[o];
        q = amax[o];
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
        tile[(2 * i + (a >> 1)) * DP_RS + (2 + 2 * sx + (a & 1)) * DP_CS + sc] = q == a ? dp : 0.f;
    }
    __syncthreads();
    // one (kx, 4 channels) step per iteration, not unrolled: its 60 weights fit the scalar registers (unrolling the
    // ten steps makes hipcc hoist all 600 scalar loads and spill ~670 SGPRs)
#pragma unroll 1
    for (int kx = 0; kx < DP_KS; ++kx) {
#pragma unroll 1
      for (int c4 = 0; c4 < DP_CC; c4 += 4) {
        f32x4 v[DP_R + DP_KS - 1];
#pragma unroll
        for (int j = 0; j < DP_R + DP_KS - 1; ++j)
          v[j] = *reinterpret_cast<const f32x4*>(&tile[(l0 + j) * DP_RS + (x + kx) * DP_CS + c4]);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          // dIn[y][x] += dConv[y + ky - 2][x + kx - 2][co] * W[co][4 - ky][4 - kx]
          const float* wc = w + ((long)(c0 + c4 + c) * DP_KS * DP_KS + (DP_KS - 1 - kx)) * DP_CI;
#pragma unroll
          for (int r = 0; r < DP_R; ++r)
#pragma unroll
            for (int ky = 0; ky < DP_KS; ++ky)
#pragma unroll
              for (int ci = 0; ci < DP_CI; ++ci)
                acc[r][ci] = fmaf(v[r + ky][c], wc[(DP_KS - 1 - ky) * DP_KS * DP_CI + ci], acc[r][ci]);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < DP_R; ++r) {
    const int y = y0 + l0 + r;
    if (y < H) {
      float* o = din + (((long)n * H + y) * DP_W + x) * DP_CI;
#pragma unroll
      for (int ci = 0; ci < DP_CI; ++ci) o[ci] = acc[r][ci];
    }
  }
}
}  // namespace

extern "C" int sd_conv2d_dgrad_pool_ok(int H, int W, int Co, int Ci, int kh, int kw, int pad) {
  return Co == DP_CO && Ci == DP_CI && kh == DP_KS && kw == DP_KS && pad == DP_KS / 2 && W == DP_W && H >= 2 &&
         H % 2 == 0;
}
extern "C" int sd_conv2d_dgrad_pool(const float* dpool, const uint8_t* amax, const float* w, float* din, int Nb, int H,
                                    int W, int Co, int Ci, int kh, int kw, int pad, sd_stream stream_) {
  if (!sd_conv2d_dgrad_pool_ok(H, W, Co, Ci, kh, kw, pad) || (long)Nb * sd_cdiv(H, DP_TH) > 0x7fffffffL)
    return SD_ESHAPE;
  if (Nb <= 0) return SD_OK;
  if (!dpool || !amax || !w || !din) return SD_EARG;
  conv_dgrad_pool_k<<<Nb * sd_cdiv(H, DP_TH), 256, 0, (hipStream_t)stream_>>>(dpool, amax, w, din, H);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

// ---------------------------------------------------------------- wide stages: split-bf16 backward contractions
// Shapes with a channel count above 128 (every older split-bf16 arm refuses them), pixel and tile counts in int range.
static bool wide3_shape(int Nb, int Hs, int Ws, int Ci, int Co, int kh, int kw) {
  if (Nb <= 0 || Hs <= 0 || Ws <= 0 || Ci <= 0 || Co <= 0 || kh <= 0 || kw <= 0) return false;
  if (Ci <= 128 && Co <= 128) return false;
  const long M = (long)Nb * Hs * Ws, K = (long)kh * kw * Ci + 1;
  return M < (1L << 30) && K < (1L << 24) && sd_cdiv(M, WIDE_BM) * sd_cdiv((long)Co, WIDE_BN) < (1L << 30);
}

// dgrad arguments as sd_conv2d_dgrad_bf16x3: Ci = dOut's channels, Co = dIn's
extern "C" int sd_conv2d_dgrad_wide3_ok(int Nb, int Hs, int Ws, int Ci, int Co, int kh, int kw, int pad) {
  return wide3_shape(Nb, Hs, Ws, Ci, Co, kh, kw) && pad >= 0 && pad < kh && pad < kw;
}

extern "C" int sd_conv2d_dgrad_wide3(const float* dout, const float* wflip, float* din, int Nb, int Hs, int Ws,
                                     int Ci, int Co, int kh, int kw, int pad, sd_stream stream_) {
  if (!sd_conv2d_dgrad_wide3_ok(Nb, Hs, Ws, Ci, Co, kh, kw, pad)) return SD_ESHAPE;
  if (!dout || !wflip || !din) return SD_EARG;
  Geom G{dout, Nb, Hs, Ws, Ci, Hs, Ws, kh, kw, pad, 0};
  GemmArgs g{};
  g.B = wflip; g.C = din; g.ldb = (long)kh * kw * Ci; g.ldc = Co;
  g.M = Nb * Hs * Ws; g.N = Co; g.K = kh * kw * Ci; g.batch = 1; g.ksplit = 1; g.kchunk = g.K;
  g.alpha = 1.f; g.beta = 0.f;
  const bool va = Ci % 4 == 0 && aligned16(dout), vb = g.K % 4 == 0 && aligned16(wflip);
  const int ntn = sd_cdiv(Co, WIDE_BN);
  const int grid = ntn * sd_cdiv(g.M, WIDE_BM);
  with_bools([&](auto VA, auto VB) {
    conv_dgrad_wide3<VA(), VB()><<<grid, 256, 0, (hipStream_t)stream_>>>(g, G, ntn);
  }, va, vb);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

// slabs of the wide bwd-weight: `request` > 0 as asked (at most one per 32-pixel k tile), else enough workgroups for
// about four per CU, no slab under 8 k tiles, at most 64; 0: the shape is not the wide arm's
extern "C" int sd_conv2d_wgrad_wide3_slabs(int Nb, int Hs, int Ws, int Ci, int Co, int kh, int kw, int request) {
  // Ci < 64 (a first stage: the 4-channel padded image): a wave's 64 im2col rows scatter over 16 taps and the f32
  // tiles are faster (measured, profiles/wide_encoder.md): not routed
  if (!wide3_shape(Nb, Hs, Ws, Ci, Co, kh, kw) || Ci < SD_WIDE3_WGRAD_MIN_CI) return 0;
  const long ktiles = sd_cdiv((long)Nb * Hs * Ws, (long)BK);
  long s = request;
  if (request <= 0) {
    const long tiles = sd_cdiv((long)Co, WIDE_BM) * sd_cdiv((long)kh * kw * Ci + 1, WIDE_BN);
    s = sd_cdiv(1024L, tiles);
    if (s > ktiles / 8) s = ktiles / 8;
    if (s > 64) s = 64;
  }
  if (s > ktiles) s = ktiles;
  return (int)(s < 1 ? 1 : s);
}

extern "C" int sd_conv2d_wgrad_wide3(const float* in, const float* dout, float* dw_db, float* workspace,
                                     long ws_floats, int slabs, int Nb, int Hs, int Ws, int Ci, int Co, int kh, int kw,
                                     int pad, const sd_wgrad_acc* acc_p, sd_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  const int ks = sd_conv2d_wgrad_wide3_slabs(Nb, Hs, Ws, Ci, Co, kh, kw, slabs);
  if (ks <= 0 || pad < 0 || pad >= kh || pad >= kw) return SD_ESHAPE;
  sd_wgrad_acc acc;
  if (!wgrad_acc_arg(acc_p, Ci, acc) || !in || !dout || !dw_db || !workspace) return SD_EARG;
  const int J = kh * kw * Ci;
  if (ws_floats < (long)ks * Co * (J + 1)) return SD_EARG;
  Geom G{in, Nb, Hs, Ws, Ci, Hs, Ws, kh, kw, pad, 0};
  GemmArgs g{};
  g.A = dout; g.lda = Co; g.C = workspace; g.ldc = J + 1; g.ws = workspace;
  g.M = Co; g.N = J + 1; g.K = Nb * Hs * Ws; g.batch = 1; g.ksplit = ks;
  g.kchunk = (int)(sd_cdiv(sd_cdiv((long)g.K, (long)ks), (long)BK) * BK);
  g.alpha = 1.f; g.beta = 0.f;
  const bool va = Co % 4 == 0 && aligned16(dout);
  const int ntn = sd_cdiv(g.N, WIDE_BN);
  const dim3 grid(ntn * sd_cdiv(Co, WIDE_BM), ks);
  with_bools([&](auto VA) { conv_wgrad_wide3<VA()><<<grid, 256, 0, s>>>(g, G, J, ntn); }, va);
  SD_LAUNCH_CHECK();
  const long total = (long)Co * (J + 1);
  slab_reduce<<<(int)((total + 63) / 64), 256, 0, s>>>(workspace, ks, total, dw_db, acc, J, Ci);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
