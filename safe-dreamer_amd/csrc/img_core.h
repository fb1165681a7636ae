// Loaders and lane helpers shared by the imagination kernels: the forward (img.hip) and the fused step backward
// (imgbwd.hip). Row-major LDS images of BM x BK (A) and BN x BK (B) tiles for the gemm16 / gemm6 main loops.
#pragma once
#include "common.h"
#include "gemm6_core.h"
#include "gemm_core.h"

namespace {
using namespace sdg;

SD_DEV f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// ------------------------------------------------------------------------------------------- A loaders
// Row-major LDS image of a BM x BK tile; thread i holds row i / 8, k-quad i % 8 (float4 along k).
template <int BM>
struct AStage {
  static constexpr int NV = (BM * BK / 4 + 255) / 256;
  f32x4 r[NV];
  SD_DEV static int row(int v) { return (threadIdx.x + 256 * v) / (BK / 4); }
  SD_DEV static int kq(int v) { return (threadIdx.x + 256 * v) % (BK / 4); }
  // static when slot v is full for every thread (hipcc cannot see threadIdx.x < 256): no branch in the k loop
  SD_DEV static bool live(int v) { return 256 * (v + 1) <= BM * BK / 4 || threadIdx.x + 256 * v < BM * BK / 4; }
  SD_DEV void store(float* lds) const {
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if (live(v)) *reinterpret_cast<f32x4*>(lds + row(v) * LDS_ROW + 4 * kq(v)) = r[v];
  }
  SD_DEV void store6(__bf16* lds) const {
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if (live(v)) split3_store(lds + row(v) * LROW6 + 4 * kq(v), r[v]);
  }
};

// Per-row rstd of the workgroup's BM rows from `np` partial sums of squares part[p*M + m] over `width` columns,
// into LDS rs[BM]. 256 threads: row = tid % BM, partial group tid / BM; all loads issued at once (MAXP per thread),
// coalesced along rows. Fixed summation order.
template <int BM, int MAXP>
SD_DEV void wg_rstd(const float* part, int np, int M, int m0, int width, float eps, float* rs, float* red) {
  constexpr int G = 256 / BM;
  const int tid = threadIdx.x, row = tid % BM, grp = tid / BM;
  const sd_rsrc rp = sd_make_rsrc(part, (long)np * M * 4);
  float v[MAXP];
#pragma unroll
  for (int k = 0; k < MAXP; ++k) {
    const int p = grp + G * k;
    v[k] = sd_bload1(rp, (p < np && m0 + row < M) ? (uint32_t)(((long)p * M + m0 + row) * 4) : SD_OOB);
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < MAXP; ++k) s += v[k];
  red[tid] = s;
  __syncthreads();
  if (tid < BM) {
    float t = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) t += red[g * BM + tid];
    rs[tid] = rsqrtf(t / (float)width + eps);
  }
  __syncthreads();
}

template <int BM>
struct APlain : AStage<BM> {
  using AStage<BM>::r;
  sd_rsrc rx;
  long ld;
  int m0, M;
  SD_DEV APlain() = default;
  SD_DEV APlain(const float* X, long ld_, int m0_, int M_, int K) : ld(ld_), m0(m0_), M(M_) {
    rx = sd_make_rsrc(X, ((long)(M - 1) * ld + K) * 4);
  }
  SD_DEV void load(int k0, int) {
#pragma unroll
    for (int v = 0; v < AStage<BM>::NV; ++v) {
      const int m = m0 + this->row(v);
      r[v] = sd_bload4(rx, m < M ? (uint32_t)(((long)m * ld + k0 + 4 * this->kq(v)) * 4) : SD_OOB);
    }
  }
};

// A(m, k) = silu(X[m][k] * rstd[m] * w[k]), rstd of the tile's rows in LDS (wg_rstd). The loads only fill
// registers; the RMSNorm + SiLU is applied when the tile is staged into LDS (store), PF k tiles later, so the
// loads stay in flight behind the MFMAs instead of being waited for at issue.
template <int BM>
struct ARms : AStage<BM> {
  using AStage<BM>::r;
  using AStage<BM>::NV;
  sd_rsrc rx;
  const float* w;
  long ld;
  int m0, M;
  float rr[NV];
  f32x4 wr[NV];
  SD_DEV ARms() = default;
  SD_DEV ARms(const float* X, long ld_, const float* w_, const float* rs, int m0_, int M_, int K)
      : w(w_), ld(ld_), m0(m0_), M(M_) {
    rx = sd_make_rsrc(X, ((long)(M - 1) * ld + K) * 4);
#pragma unroll
    for (int v = 0; v < NV; ++v) rr[v] = rs[this->row(v)];
  }
  SD_DEV void load(int k0, int) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int gk = k0 + 4 * this->kq(v), m = m0 + this->row(v);
      r[v] = sd_bload4(rx, m < M ? (uint32_t)(((long)m * ld + gk) * 4) : SD_OOB);
      wr[v] = ld4(w + gk);
    }
  }
  SD_DEV f32x4 val(int v) const {
    f32x4 y;
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = siluf_(r[v][j] * rr[v] * wr[v][j]);
    return y;
  }
  SD_DEV void store(float* lds) const {
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if (this->live(v)) *reinterpret_cast<f32x4*>(lds + this->row(v) * LDS_ROW + 4 * this->kq(v)) = val(v);
  }
  SD_DEV void store6(__bf16* lds) const {
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if (this->live(v)) split3_store(lds + this->row(v) * LROW6 + 4 * this->kq(v), val(v));
  }
};

// B operand: rows of a k-contiguous weight matrix; local row lr -> global row base + (lr / seg) * stride + lr % seg
template <int BN>
struct BRows {
  static constexpr int NV = (BN * BK / 4 + 255) / 256;
  f32x4 r[NV];
  const float* W;
  long ld;
  int base, seg, stride, nrows;  // rows >= nrows read as 0 (the actor's output weight has only 2A or A rows)
  SD_DEV BRows() = default;
  SD_DEV BRows(const float* W_, long ld_, int base_, int seg_, int stride_, int nrows_ = 1 << 30)
      : W(W_), ld(ld_), base(base_), seg(seg_), stride(stride_), nrows(nrows_) {}
  SD_DEV void load(int k0, int) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int i = threadIdx.x + 256 * v;
      if (256 * (v + 1) <= BN * BK / 4 || i < BN * BK / 4) {
        const int lr = i / (BK / 4), kq = i % (BK / 4);
        const long gr = base + (lr / seg) * stride + lr % seg;
        r[v] = gr < nrows ? ld4(W + gr * ld + k0 + 4 * kq) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }
  SD_DEV void store(float* lds) const {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int i = threadIdx.x + 256 * v;
      if (256 * (v + 1) <= BN * BK / 4 || i < BN * BK / 4)
        *reinterpret_cast<f32x4*>(lds + (i / (BK / 4)) * LDS_ROW + 4 * (i % (BK / 4))) = r[v];
    }
  }
  SD_DEV void store6(__bf16* lds) const {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int i = threadIdx.x + 256 * v;
      if (256 * (v + 1) <= BN * BK / 4 || i < BN * BK / 4)
        split3_store(lds + (i / (BK / 4)) * LROW6 + 4 * (i % (BK / 4)), r[v]);
    }
  }
};

// Wave (wr, wc) of a BM x BN tile owns rows wr*16 + 4q + r and columns wc*WN + 16j + l16 (gemm16_mainloop layout).
struct Lane {
  int l16, q, wr, wc;
};
template <int BN, int WN>
SD_DEV Lane lane_ids() {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  return Lane{lane & 15, lane >> 4, wave / (BN / WN), wave % (BN / WN)};
}

}  // namespace
