// Fused imagination: Dreamer._imagine (dreamer.py:673-692) = for each of H1 steps: actor MLP on feat = [stoch, deter]
// (networks.py:313-377) -> action sample (bounded normal / one-hot) -> RSSM.img_step (rssm.py:180-187:
// Deter.forward rssm.py:36-75 + prior img_net + one-hot sample). N (= B*T) independent rows per step.
//
// 9 launches per step (the per-op path took ~28): each launch is a row-tiled fp32-accurate MFMA contraction
// (v_mfma_f32_16x16x4_f32, or six bf16 MFMAs per fp32 product, gemm6_core.h) with
//   * A loaders that apply the previous layer's RMSNorm + SiLU while staging K-tiles into LDS — the per-row rstd
//     comes from row partial sums of squares that the PRODUCER's epilogue wrote (one float per row per 16*TN
//     output columns), so no normalised activation is ever materialised and no norm launch exists;
//   * epilogues that fuse the bias, those row partials, the GRU gate, the unimix one-hot prior sampler, and the
//     whole action branch (bounded-normal / one-hot action, action_norm, _dyn_in2 Linear + RMSNorm + SiLU);
//   * independent contractions that share an A operand grouped into one launch (actor layer 0 with _dyn_in1,
//     img_net_0 with the next step's _dyn_in0).
// Results land directly in the reference's (H1, N, F) feat and (H1, N, A) action layouts.
#include <cstdlib>

#include "common.h"
#include "dist_core.h"
#include "gemm6_core.h"
#include "gemm_core.h"
#include "img_core.h"
#include "philox.h"
#include "sdhip.h"


namespace {
using namespace sdg;

// (ld4, the A loaders AStage / APlain / ARms with wg_rstd, BRows, Lane / lane_ids: img_core.h)
// B operand from a pre-split weight image (k_presplit6): the BN x 32 tile (ct, kt) is stored as its three bf16
// planes, [row][a0 32 | a1 32 | a2 32] (192 B a row), contiguous per tile, so a k tile is one coalesced read of
// 12 KB and store6 copies it into the LDS image in 16-B pieces with no VALU. The planes are split3_store's, so the
// contraction is bit-identical to BRows + store6 on the fp32 weight.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int PRE_ROW = 3 * BK6;  // bf16 per row of a pre-split tile
// TH: the image's tile height when it is taller than the BN rows read (rows sub .. sub + BN - 1 of each TH-row tile)
template <int BN, int TH = BN>
struct BPre6 {
  static constexpr int PCS = BN * PRE_ROW / 8, NV = (PCS + 255) / 256;  // 16-B pieces per tile
  u32x4 r[NV];
  const __bf16* tile0;
  SD_DEV BPre6() = default;
  SD_DEV BPre6(const __bf16* pre, int ct, int nkt, int kt0, int sub = 0)
      : tile0(pre + (((long)ct * nkt + kt0) * TH + sub) * PRE_ROW) {}
  SD_DEV static bool live(int v) { return 256 * (v + 1) <= PCS || threadIdx.x + 256 * v < PCS; }
  SD_DEV void load(int k0, int) {
    const __bf16* t = tile0 + (long)(k0 / BK6) * TH * PRE_ROW;
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if (live(v)) r[v] = *reinterpret_cast<const u32x4*>(t + (threadIdx.x + 256 * v) * 8);
  }
  SD_DEV void store6(__bf16* lds) const {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int i = threadIdx.x + 256 * v;
      if (live(v)) *reinterpret_cast<u32x4*>(lds + (i / (PRE_ROW / 8)) * LROW6 + (i % (PRE_ROW / 8)) * 8) = r[v];
    }
  }
};
// W (rows, K) fp32, k contiguous -> the BPre6 image of BN-row column tiles: tile (n / BN, k / 32), row n % BN.
// One thread per (row, k quad). rows % BN == 0, K % 32 == 0 (the caller checks).
// _dyn_gru's weight for k_gate: tile ct = 32 deter columns c0 = 32 ct of block g = c0 / Dg, its 96 rows the r / c / u
// gate rows g*3Dg + {0, Dg, 2Dg} + c0 % Dg + (0..31) of Wg viewed as (3D, Dg); K = Dg.
__global__ __launch_bounds__(256) void k_presplit6_gate(const float* Wg, int D, int Dg, __bf16* out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int nq = Dg / 4;
  if (i >= (long)3 * D * nq) return;
  const int rr = (int)(i / nq), k = 4 * (int)(i % nq), nkt = Dg / BK6;  // rr: row of the (3D) tile-ordered image
  const int ct = rr / 96, lr = rr % 96, c0 = ct * 32, g = c0 / Dg;
  const long wrow = (long)g * 3 * Dg + (lr / 32) * Dg + c0 % Dg + lr % 32;
  split3_store(out + (((long)ct * nkt + k / BK6) * 96 + lr) * PRE_ROW + k % BK6, ld4(Wg + wrow * Dg + k));
}
template <int BN>
__global__ __launch_bounds__(256) void k_presplit6(const float* W, int rows, int K, __bf16* out, long ldw = 0) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int nq = K / 4;
  if (i >= (long)rows * nq) return;
  const int n = (int)(i / nq), k = 4 * (int)(i % nq), nkt = K / BK6;
  split3_store(out + (((long)(n / BN) * nkt + k / BK6) * BN + n % BN) * PRE_ROW + k % BK6,
               ld4(W + (long)n * (ldw ? ldw : K) + k));
}

// Pre-split ACTIVATION images: the same BPre6 tile layout for a (rows, K) activation — tile (row / 64,
// col / 32), row % 64 — written once by the producer, so the k_hid tiles that read a row (D / 64 column tiles of it)
// copy its planes instead of each splitting it again (split3 of the same fp32 value: bit-identical operands).
SD_DEV long pre_off(long row, int col, int K) {
  return (((row >> 6) * (K / BK6) + col / BK6) * 64 + (row & 63)) * PRE_ROW + (col % BK6);
}
// 4 consecutive columns (col % 4 == 0) of one row
SD_DEV void pre_store4(__bf16* img, long row, int col, int K, f32x4 v) { split3_store(img + pre_off(row, col, K), v); }
// the image of a strided (rows, K) fp32 matrix (feats(0)'s deter at the first step)
__global__ __launch_bounds__(256) void k_presplit_rows(const float* X, long ldx, int rows, int K, __bf16* out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int nq = K / 4;
  if (i >= (long)rows * nq) return;
  const long r = i / nq;
  const int k = 4 * (int)(i % nq);
  pre_store4(out, r, k, K, ld4(X + r * ldx + k));
}

// ------------------------------------------------------------------------------------------- contraction
// Main loop per kernel (measured, imagination alone, N = 1024): k_hid and k_gate on the single-stage bf16x6 loop
// (gemm6_mainloop_1s; gemm6_core.h: fp32-accurate, 2.67x the fp32 MFMA rate), k_lin on the fp32 fragment-prefetch loop
// (gemm16_mainloop_fp: LDS reads of tile k+1 issued ahead of tile k's MFMAs), k_lin6 on its bf16x6 form
// (gemm6_mainloop_fp). These launches are bound by operand traffic and per-launch latency, not by the MFMA pipe
// (tools/pmc_table.py: k_hid MFMA busy ~0.45); DESIGN.md § 4.3 keeps the comparisons.
static_assert(BK == BK6, "tile depth");
// prefetch depths: register sets of each loader, which the main loops take as arrays built from one prototype
// (op_sets in k_lin / k_lin6, a loop in place in hid_seg / k_gate: each is the form whose code object was measured —
// hipcc orders a few instructions differently between the two)
constexpr int KH_PF = 1, KG_PF = 1, KL_PF = 2;
template <int PF, class Op>
SD_DEV void op_sets(Op (&s)[PF], const Op& o) {
#pragma unroll
  for (int u = 0; u < PF; ++u) s[u] = o;
}

// ------------------------------------------------------------------------------------------- epilogue helpers

// out[m][n] = acc + bias[n] (+ add[m][n]); part[(n / PW) * M + m] = sum over each PW-column group of out^2 (the
// consumers' wg_rstd reads width / PW partials per row whatever the producer's tile shape: PW = 32 for the U-wide
// MLP layers, 64 for dyn_hid). WN % PW == 0.
template <int BM, int BN, int WN, int PW = 32>
SD_DEV void ep_bias_part(const f32x4 (&acc)[1][WN / 16], const float* bias, float* out, long ldo, float* part, int M,
                         int m0, int n0, const float* add = nullptr, const float* bvals = nullptr) {
  constexpr int TN = WN / 16, TP = PW / 16;
  static_assert(WN % PW == 0, "whole row-partial groups per wave");
  const Lane L = lane_ids<BN, WN>();
  float ss[WN / PW][4] = {};
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + L.wc * WN + 16 * j + L.l16;
    const float bv = bvals ? bvals[j] : bias ? bias[n] : 0.f;  // (bvals: the bias values, loaded by the caller)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + L.wr * 16 + 4 * L.q + r;
      float v = acc[0][j][r] + bv;
      if (add && m < M) v += add[(long)m * ldo + n];
      if (m < M) out[(long)m * ldo + n] = v;
      ss[j / TP][r] += v * v;
    }
  }
#pragma unroll
  for (int p = 0; p < WN / PW; ++p)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float s = group_sum<16>(ss[p][r]);
      const int m = m0 + L.wr * 16 + 4 * L.q + r;
      if (L.l16 == 0 && part && m < M) part[(long)((n0 + L.wc * WN) / PW + p) * M + m] = s;
    }
}

// ------------------------------------------------------------------------------------------- kernels
// XCD-aware column-tile order for the block-diagonal (G blocks) layers: workgroups are dealt to the 8 XCDs round
// robin by linear id, and gridDim.x is a multiple of 8, so an XCD runs the x = xcd (mod 8) column tiles of every row
// tile. Mapping x -> tile (x % G) * tpb + x / G puts all tiles of block g = x % G on one XCD (G = 8): that XCD's L2
// then serves the block's input columns and weights to all of them, instead of every XCD streaming every block.
SD_DEV int xcd_col(int x, int nx, int tpb) {
  const int G = nx / tpb;
  return (x % G) * tpb + x / G;
}
// XCD-aware tile order for the grouped plain GEMMs (k_lin, grid (col tiles, row tiles, problems)): the 8 XCDs form a
// 4 (row groups) x 2 (column groups over all problems) grid, so an XCD's L2 serves a quarter of A and half of the
// weights instead of all of A (dispatch order deals linear ids round robin to the XCDs). Identity when the grid does
// not split that way.
SD_DEV void xcd_tile(int& tx, int& ty, int& tz) {
  const int nx = gridDim.x, ny = gridDim.y, cols = nx * gridDim.z;
  if (ny % 4 || cols % 2) return;
  const int id = blockIdx.x + nx * (blockIdx.y + ny * blockIdx.z), xcd = id % 8, slot = id / 8;
  const int R4 = ny / 4, C2 = cols / 2;
  const int row = (xcd >> 1) * R4 + slot % R4, col = (xcd & 1) * C2 + slot / R4;
  tx = col % nx;
  ty = row;
  tz = col / nx;
}

struct LinProb {
  const float* A;
  long lda;
  int K;
  const float* W;  // (N, K) k-contiguous (ld = ldw)
  long ldw;
  const float* bias;
  float* out;
  long ldo;
  float* part;
  const float* add;  // optional (M, ldo) term added before the row partials (a K-split layer's first part)
};

// tile of the step's three (N, D) x (D, U) contractions (img_net_0 + _dyn_in0 + actor layer 0's deter part)
constexpr int KL3_BM = 32, KL3_BN = 32;
// tile of the step's K = S*Kd launch (actor layer 0's stoch part + _dyn_in1)
constexpr int KL2_BN = 32;
constexpr int KL2_WN = KL2_BN / 2, KL2_PW = KL2_WN < 32 ? KL2_WN : 32;
constexpr int KL3_WN = KL3_BN / (4 / (KL3_BM / 16)), KL3_PW = KL3_WN < 32 ? KL3_WN : 32;  // its row-partial width
// Every producer of a U = 256 wide hidden row (k_lin / k_lin6 / k_lin6_areg, k_onehot_lin, k_rmslin_rw) writes one
// row partial per 16 columns, and the register-tile and per-row consumers (RTile, k_action_rows) read at most 16
constexpr int ROW_PW = 16;
static_assert(KL2_PW == ROW_PW && KL3_PW == ROW_PW, "16 row partials per 256-column hidden row");
// grouped plain-A linear layers (N = 256 each): out = A . W^T + b (+ add), with row partials. grid (N/BN, M/BM, nprob)
template <int BM, int BN>
__global__ __launch_bounds__(256) void k_lin(LinProb p0, LinProb p1, LinProb p2, int M, Tr tr) {
  SD_TR_BEGIN
  constexpr int WN = BN / (4 / (BM / 16));
  int tx = blockIdx.x, ty = blockIdx.y, tz = blockIdx.z;
  xcd_tile(tx, ty, tz);
  const LinProb p = tz == 0 ? p0 : (tz == 1 ? p1 : p2);
  const int n0 = tx * BN, m0 = ty * BM;
  APlain<BM> la[KL_PF];
  BRows<BN> lb[KL_PF];
  op_sets(la, APlain<BM>(p.A, p.lda, m0, M, p.K));
  op_sets(lb, BRows<BN>(p.W, p.ldw, n0, BN, 0));
  f32x4 acc[1][WN / 16];
  SD_TR(1)
  gemm16_mainloop_fp<BM, BN, 16, WN, KL_PF>(la, lb, 0, p.K, acc);
  SD_TR(2)
  ep_bias_part<BM, BN, WN, (WN < 32 ? WN : 32)>(acc, p.bias, p.out, p.ldo, p.part, M, m0, n0, p.add);
  SD_TR_END(tr.p, tr.slot)
}

// k_lin on the bf16x6 path with both operands pre-split: A = deter' from the image k_gate already wrote for
// the next k_hid (64-row tiles), B = the three weights' images (built once per imagination), so the main loop only
// copies bf16 planes into LDS (no split VALU) and runs at the bf16 MFMA rate (six products per fp32 product:
// fp32-accurate, gemm6_core.h). Same outputs and row partials (KL3_PW wide) as k_lin<KL3_BM, KL3_BN>.
// k_lin6 row tile: 32 (2 x 2 waves, half of each 64-row image tile: 768 workgroups, 3 per CU), not 64 (4 waves x 16
// rows: 384 workgroups, two on half the CUs) — step trace 37.8 -> 33.1 us, r04y
constexpr int KL6_BM = 32;
template <int BM, int BN>
__global__ __launch_bounds__(256) void k_lin6(const __bf16* aimg, int K, const __bf16* w0, const __bf16* w1,
                                              const __bf16* w2, LinProb p0, LinProb p1, LinProb p2, int M, Tr tr) {
  SD_TR_BEGIN
  constexpr int WN = BN / (4 / (BM / 16));
  static_assert(WN % KL3_PW == 0 && BM <= 64, "row partials; rows of one 64-row image tile");
  int tx = blockIdx.x, ty = blockIdx.y, tz = blockIdx.z;
  xcd_tile(tx, ty, tz);
  const LinProb p = tz == 0 ? p0 : (tz == 1 ? p1 : p2);
  const __bf16* wimg = tz == 0 ? w0 : (tz == 1 ? w1 : w2);
  const int n0 = tx * BN, m0 = ty * BM;
  f32x4 acc[1][WN / 16];
  SD_TR(1)
  BPre6<BM, 64> la[KL_PF];
  BPre6<BN> lb[KL_PF];
  op_sets(la, BPre6<BM, 64>(aimg, m0 / 64, K / BK6, 0, m0 % 64));
  op_sets(lb, BPre6<BN>(wimg, tx, K / BK6, 0));
  gemm6_mainloop_fp<BM, BN, 16, WN, KL_PF>(la, lb, 0, K, acc);
  SD_TR(2)
  ep_bias_part<BM, BN, WN, KL3_PW>(acc, p.bias, p.out, p.ldo, p.part, M, m0, n0, p.add);
  SD_TR_END(tr.p, tr.slot)
}

// The step's K = S*Kd contractions (actor layer 0's stoch part + _dyn_in1) read a straight-through one-hot sample:
// every categorical holds one nonzero (the sampler writes ((k == idx) - ys) + ys: exactly 0 off the index). So
// out[m] = b + add[m] + sum_s v_s WT[s*Kd + idx_s] — a gather of S rows of the pre-transposed weight WT (SK, U) per
// row, not a dense (N, SK) x (SK, U) GEMM. One wave per row, 4 columns per lane (U = 256); lane s finds categorical
// s's nonzero; the S row loads are issued in batches of OH_BATCH before their FMAs. A row with a categorical holding more
// than one nonzero takes the exact dense loop over all SK entries instead. Row partials per 16 columns, as k_lin's.
// The two one-hot problems of a step are two grid rows (blockIdx.y), so both gathers are in flight at once.
constexpr int OH_BATCH = 32;  // weight-row loads issued before their FMAs
struct OneHotProb {
  const float* WT;  // (SK, U) transposed weight
  const float* bias;
  const float* add;  // optional (M, U)
  float* out;        // (M, U)
  float* part;       // (U / 16, M)
  const float* nw;   // optional: RMSNorm weight -> img = pre-split image of silu(rms(out) * nw)
  __bf16* img;
  float eps;
};
__global__ __launch_bounds__(256) void k_onehot_lin(const float* X, long ldx, int SK, int Kd, OneHotProb p0,
                                                    OneHotProb p1, int nprob, int M, Tr tr) {
  SD_TR_BEGIN
  constexpr int U = 256;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long m = (long)blockIdx.x * 4 + wave;
  if (m >= M) return;
  const int S = SK / Kd;
  const float* x = X + m * ldx;
  // lane s < S: categorical s's first nonzero (index, value) and whether it holds another
  int idx = 0, many = 0;
  float val = 0.f;
  if (lane < S) {
    int cnt = 0;
    for (int j = 0; j < Kd; j += 4) {
      const f32x4 q = ld4(x + lane * Kd + j);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (q[e] != 0.f) {
          if (cnt == 0) { idx = j + e; val = q[e]; }
          ++cnt;
        }
    }
    many = cnt > 1;
  }
  const bool dense = __any(many);
  SD_TR(1)
  const int c = 4 * lane;
  const OneHotProb& p = blockIdx.y == 0 ? p0 : p1;  // one problem per workgroup row of the grid (nprob rows)
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (!dense) {
    for (int s0 = 0; s0 < S; s0 += OH_BATCH) {
      f32x4 w[OH_BATCH];
      float v[OH_BATCH];
#pragma unroll
      for (int u = 0; u < OH_BATCH; ++u) {
        const int s = s0 + u < S ? s0 + u : S - 1;
        const int k = s * Kd + __shfl(idx, s, 64);
        v[u] = s0 + u < S ? __shfl(val, s, 64) : 0.f;
        w[u] = ld4(p.WT + (long)k * U + c);
      }
#pragma unroll
      for (int u = 0; u < OH_BATCH; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += v[u] * w[u][e];
    }
  } else {
    for (int k = 0; k < SK; ++k) {
      const float xv = x[k];
      if (xv != 0.f) {
        const f32x4 w = ld4(p.WT + (long)k * U + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += xv * w[e];
      }
    }
  }
  const f32x4 b = p.bias ? ld4(p.bias + c) : f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 a = p.add ? ld4(p.add + m * U + c) : f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = acc[e] + b[e] + a[e];
  *reinterpret_cast<f32x4*>(p.out + m * U + c) = o;
  float ss = o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3];
  ss += __shfl_xor(ss, 1, 64);
  ss += __shfl_xor(ss, 2, 64);
  if ((lane & 3) == 0 && p.part) p.part[(long)(lane >> 2) * M + m] = ss;
  if (p.img) {  // the row's normalised output, split once for k_hid (a wave holds the whole row)
    // rstd exactly as k_hid's wg_rstd<64, 8> forms it from these 16 partials (lane 4 p holds partial p): 4 groups
    // g of partials g, g + 4, g + 8, g + 12, summed in that order, then the groups in order -> bit-identical x1
    float pp[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) pp[q] = __shfl(ss, 4 * q, 64);
    float tsum = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float sg = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) sg += pp[g + 4 * k];
      tsum += sg;
    }
    const float rs = rsqrtf(tsum / (float)U + p.eps);
    const f32x4 w = ld4(p.nw + c);
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = siluf_(o[e] * rs * w[e]);
    pre_store4(p.img, m, c, U, y);
  }
  SD_TR(2)
  SD_TR_END(tr.p, tr.slot)
}
// WT (K, U) = W[:, 0:K]^T for a (U, ldw) weight
__global__ __launch_bounds__(256) void k_transpose_w(const float* W, long ldw, int U, int K, float* WT) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)U * K) return;
  const int k = (int)(i / U), c = (int)(i % U);
  WT[i] = W[(long)c * ldw + k];
}

// ------------------------------------------------------------------------------------------- 16 x 64 register tiles
// The short-K (K = U = 256) layers on 16-row tiles — the actor / img_net hidden layers (k_rmslin_rw) and the prior
// logits (k_prior_rw) — measured as latency chains when run as an LDS-staged k loop of 8 tiles with a barrier each
// (the former k_rmslin / k_prior). Here each workgroup
// stages the RMSNorm + SiLU'd A panel (16 rows x K, from the producer's row partials) into LDS ONCE, every wave loads
// its weight fragments straight into registers at entry (column tile w % 4, K part w / 4: K / KS per wave), the MFMAs
// run from registers + LDS with no further barrier, and the KS k-parts are summed in a fixed order through LDS.
// v_mfma_f32_16x16x4_f32 (exact fp32 products): lane (l16, q) supplies k = 16c + 4q + j at MFMA j of chunk c.
template <int NWV>
struct RTile {
  static constexpr int U = 256, KS = NWV / 4, KP = U / KS, NCH = KP / 16, LDP = U + 4;
  f32x4 b[NCH];
  f32x4 acc;
  // weight rows of this wave's column tile (n0 + 16 (w % 4) + l16), its K part
  SD_DEV void load_w(const float* W, long ldw, int n0) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l16 = lane & 15, q = lane >> 4;
    const float* p = W + (long)(n0 + 16 * (w % 4) + l16) * ldw + (w / 4) * KP + 4 * q;
#pragma unroll
    for (int c = 0; c < NCH; ++c) b[c] = ld4(p + 16 * c);
  }
  // panel P[16][LDP] = silu(X[m0 + r] * rstd_r * nw), rstd from np <= 16 partials part[p * M + m]; threads 0..255:
  // row tid / 16, 16 columns each (the row's 16 threads reduce its partials: no barrier before the norm)
  // the panel's operands in registers (threads 0..255): stage_load issues the loads, stage_store normalises and
  // writes P — split so a caller can issue its weight loads in between (k_rmslin_rw) and the panel does not wait on
  // them (loads complete in issue order)
  struct Panel {
    f32x4 x[4], w[4];
    float pv;
    bool pok;  // pv is one of the np partials (else a clamped duplicate, masked in stage_store)
  };
  SD_DEV static void stage_load(Panel& q, const float* X, long ldx, const float* nw, const float* part, int np, int M,
                                int m0) {
    // unconditional loads (rows past M read row M - 1, partials past np read partial np - 1; stage_store masks
    // them): a "cond ? load : 0" made hipcc branch around the load and drain the vector-memory queue at the join
    const int tid = threadIdx.x;
    if (tid < 256) {
      const int r = tid >> 4, j = tid & 15;
      const long m = m0 + r < M ? m0 + r : M - 1;
      q.pv = part[(long)(j < np ? j : np - 1) * M + m];
      q.pok = j < np;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        q.x[i] = ld4(X + m * ldx + 16 * j + 4 * i);
        q.w[i] = ld4(nw + 16 * j + 4 * i);
      }
    }
  }
  SD_DEV static void stage_store(const Panel& q, float* P, int M, int m0, float eps) {
    const int tid = threadIdx.x;
    if (tid < 256) {
      const int r = tid >> 4, j = tid & 15;
      const bool rv = m0 + r < M;
      const float rs = rsqrtf(group_sum<16>(q.pok ? q.pv : 0.f) / (float)U + eps);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = rv ? siluf_(q.x[i][e] * rs * q.w[i][e]) : 0.f;
        *reinterpret_cast<f32x4*>(P + r * LDP + 16 * j + 4 * i) = y;
      }
    }
  }
  SD_DEV static void stage(float* P, const float* X, long ldx, const float* nw, const float* part, int np, int M,
                           int m0, float eps) {
    Panel q;
    stage_load(q, X, ldx, nw, part, np, M, m0);
    stage_store(q, P, M, m0, eps);
  }
  SD_DEV void mma(const float* P) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l16 = lane & 15, q = lane >> 4;
    acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* a = P + l16 * LDP + (w / 4) * KP + 4 * q;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const f32x4 av = ld4(a + 16 * c);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], b[c][j], acc, 0, 0, 0);
    }
  }
  // sum of the KS k-parts into tile T[16][64 + 1] (row 4q + r, column 16 (w % 4) + l16), in k-part order
  SD_DEV void reduce(float* red, float* T) const {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l16 = lane & 15, q = lane >> 4;
    if (KS > 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(w * 4 + r) * 64 + lane] = acc[r];
      __syncthreads();
      if (w < 4) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = red[(w * 4 + r) * 64 + lane];
#pragma unroll
          for (int k = 1; k < KS; ++k) v += red[((w + 4 * k) * 4 + r) * 64 + lane];
          T[(4 * q + r) * 65 + 16 * w + l16] = v;
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) T[(4 * q + r) * 65 + 16 * w + l16] = acc[r];
    }
    __syncthreads();
  }
};

// out = silu(rms(X)) . W^T + b (MLP hidden layer after the first) on RTile<8>: 512 threads, grid (U / 64, M / 16);
// 16-column row partials (part[p * M + m], p = column / 16). The A panel's loads are issued before the weight loads,
// so its normalisation waits only on them (k_prior_rw would spill doing so: 64 VGPRs).
__global__ __launch_bounds__(512) void k_rmslin_rw(const float* X, const float* nw, const float* part_in, int np,
                                                   const float* W, const float* bias, float* out, float* part, int M,
                                                   float eps, Tr tr) {
  SD_TR_BEGIN
  using RT = RTile<8>;
  __shared__ __attribute__((aligned(16))) float P[16 * RT::LDP];
  __shared__ float red[8 * 4 * 64];
  __shared__ float T[16 * 65];
  const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 16;
  RT rt;
  typename RT::Panel q;
  RT::stage_load(q, X, RT::U, nw, part_in, np, M, m0);
  rt.load_w(W, RT::U, n0);
  RT::stage_store(q, P, M, m0, eps);
  __syncthreads();
  SD_TR(1)
  rt.mma(P);
  rt.reduce(red, T);
  SD_TR(2)
  const int tid = threadIdx.x;
  if (tid < 256) {  // row tid / 16, columns 4 (tid % 16) .. +3
    const int r = tid >> 4, j = tid & 15;
    const long m = m0 + r;
    const f32x4 bv = ld4(bias + n0 + 4 * j);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = T[r * 65 + 4 * j + e] + bv[e];
    if (m < M) *reinterpret_cast<f32x4*>(out + m * RT::U + n0 + 4 * j) = v;
    float ss = v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    ss += __shfl_xor(ss, 1, 64);
    ss += __shfl_xor(ss, 2, 64);  // 4 threads = 16 columns
    if ((j & 3) == 0 && m < M) part[(long)(n0 / 16 + (j >> 2)) * M + m] = ss;
  }
  SD_TR_END(tr.p, tr.slot)
}

// k_hid tiling: rows per workgroup, register budget (waves per SIMD)
constexpr int KH_BM = 64, KH_WAVES = 2;
constexpr int KH_WN = 64 / (4 / (KH_BM / 16)), KH_PW = KH_WN < 64 ? KH_WN : 64;  // hp row-partial width
// one K segment of k_hid on the single-stage bf16x6 loop
template <int BM, int BN, int WN, class OpA, class OpB>
SD_DEV void hid_seg(const OpA& a0, const OpB& b0, int K, f32x4 (&acc)[1][WN / 16], bool accumulate) {
  OpA la[KH_PF];
  OpB lb[KH_PF];
#pragma unroll
  for (int u = 0; u < KH_PF; ++u) {
    la[u] = a0;
    lb[u] = b0;
  }
  gemm6_mainloop_1s<BM, BN, 16, WN, KH_PF>(la, lb, 0, K, acc, accumulate);
}

// hp = BlockLinear(dyn_hid_0)([h_g | x0 | x1 | x2]) + bh with x0 = silu(rms(x0p)), x1 = silu(rms(x1p)) applied by the
// A loaders (rssm.py:52-63): four main loops over the input segments accumulate into one tile. BM = BN = 64,
// grid (D/64, M/64); row partials per 64 columns (D/64 of them) for the gate norm.
template <bool APRE>
__global__ __launch_bounds__(256, KH_WAVES) void k_hid(sd_imagine d, const float* h, long ldh, const float* x0p, const float* x1p,
                                             const float* px0, const float* px1, int npx0, int npx1, const float* x2, float* hp,
                                             float* ph, const __bf16* wh6, const __bf16* himg, const __bf16* x1img,
                                             const __bf16* x2img, Tr tr) {
  SD_TR_BEGIN
  constexpr int BM = KH_BM, BN = 64, WN = BN / (4 / (BM / 16));
  static_assert(!APRE || BM == 64, "pre-split activation images are in 64-row tiles");
  __shared__ float rs0[BM], rs1[BM], red[256];
  const int Dg = d.D / d.G, U = d.U, Ig = Dg + 3 * U, M = d.N;
  const int n0 = xcd_col(blockIdx.x, gridDim.x, Dg / BN) * BN, m0 = blockIdx.y * BM, g = n0 / Dg;
  wg_rstd<BM, 8>(px0, npx0, M, m0, U, d.eps, rs0, red);
  if (!APRE) wg_rstd<BM, 8>(px1, npx1, M, m0, U, d.eps, rs1, red);
  SD_TR(1)
  const int ct = n0 / BN, nkt = Ig / BK6;
  // the four K segments of [h_g | x0 | x1 | x2]: B from _dyn_hid's once-per-imagination pre-split image
  auto bseg = [&](int k0) { return BPre6<BN>(wh6, ct, nkt, k0 / BK6); };
  f32x4 acc[1][WN / 16];
  if constexpr (APRE) {  // h, x1 and x2 from their producers' pre-split images (64-row tiles of m0 / 64)
    hid_seg<BM, BN, WN>(BPre6<BM>(himg, m0 / BM, d.D / BK6, g * Dg / BK6), bseg(0), Dg, acc, false);
  } else {
    const APlain<BM> a0(h + (long)g * Dg, ldh, m0, M, Dg);
    hid_seg<BM, BN, WN>(a0, bseg(0), Dg, acc, false);
  }
  {
    const ARms<BM> a0(x0p, U, d.n0, rs0, m0, M, U);
    hid_seg<BM, BN, WN>(a0, bseg(Dg), U, acc, true);
  }
  if constexpr (APRE) {
    hid_seg<BM, BN, WN>(BPre6<BM>(x1img, m0 / BM, U / BK6, 0), bseg(Dg + U), U, acc, true);
    hid_seg<BM, BN, WN>(BPre6<BM>(x2img, m0 / BM, U / BK6, 0), bseg(Dg + 2 * U), U, acc, true);
  } else {
    {
      const ARms<BM> a0(x1p, U, d.n1, rs1, m0, M, U);
      hid_seg<BM, BN, WN>(a0, bseg(Dg + U), U, acc, true);
    }
    {
      const APlain<BM> a0(x2, U, m0, M, U);
      hid_seg<BM, BN, WN>(a0, bseg(Dg + 2 * U), U, acc, true);
    }
  }
  SD_TR(2)
  ep_bias_part<BM, BN, WN, KH_PW>(acc, d.bh, hp, d.D, ph, M, m0, n0);
  SD_TR_END(tr.p, tr.slot)
}

// k_hid on register A operands: the same 64 x 64 tile, bf16x6 products and k order as k_hid<true>
// (bit-identical), restructured around what bounds it. k_hid<true> runs its four K segments as four single-stage loops
// that stage A and B through LDS (two barriers per k tile, LDS writes and reads serialised with the MFMAs: mma phase
// ~28 us of a 36 us launch, MFMA busy ~0.3, and unchanged when every workgroup reads one tile's operands —
// profiles/r05n: not the L2 -> CU traffic). Here wave w's A operand is its own 16 rows, so each lane loads its
// fragment (row l16, k 8q..8q+7 of each plane) straight from the producers' pre-split images into registers — deter
// (k_gate), x0 (k_action_rows), x1 (k_onehot_lin), x2 (k_action_rows) — and only B (the weight tile the four waves
// share) goes through a double-buffered LDS stage; the whole K (NKT = Dg/32 + 24 tiles) is one fully unrolled loop
// with A two tiles ahead in three register sets, B's next tile stored between this tile's MFMAs, one barrier per tile.
// Step trace (profiles/r05s): k_hid 35.4 -> 27.0 us per step, the imagination step 149.7 -> 142.8 us; update A/B
// 11.09 -> 11.01 ms. (Measured against it, r05p / r05r: 32-row waves — 2 x 2 waves on 64 x 64, or 4 x 2 on 128 x 64
// tiles, B fragments reused by two row tiles — run slower, 36.4 / 33.6 vs 28.8 us: their fragment-shaped A loads
// double per lane.)
template <int NKT>
__global__ __launch_bounds__(256, 2) void k_hid_areg(sd_imagine d, float* hp, float* ph, const __bf16* wh6,
                                                     const __bf16* himg, const __bf16* x0img, const __bf16* x1img,
                                                     const __bf16* x2img, Tr tr) {
  SD_TR_BEGIN
  constexpr int BM = 64, BN = 64, TN = 4, NH = NKT - 24;  // NH: deter tiles (Dg / 32); 8 tiles each of x0 / x1 / x2
  constexpr int STG = BN * LROW6, BP = BN * PRE_ROW / 8 / 256;  // LDS stage (bf16); 16-B B pieces per thread
  constexpr int NS = 2;  // B's LDS stages
  static_assert(BN * PRE_ROW / 8 == 256 * BP, "whole B pieces per thread");
  __bf16* smem = sd_smem6<NS * STG>();
  const int Dg = d.D / d.G, M = d.N;
  const int n0 = xcd_col(blockIdx.x, gridDim.x, Dg / BN) * BN, m0 = blockIdx.y * BM, g = n0 / Dg;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q = lane >> 4;
  SD_TR(1)
  // this lane's A row in the 64-row image tiles (tile m0 / 64), plane offsets 0 / 32 / 64 at k 8q
  const long rt = m0 / 64, lrow = (long)(16 * wave + l16) * PRE_ROW + 8 * q;
  const __bf16* ah = himg + (rt * (d.D / BK6) + (long)g * Dg / BK6) * 64 * PRE_ROW + lrow;
  const __bf16* a0 = x0img + rt * 8 * 64 * PRE_ROW + lrow;
  const __bf16* a1 = x1img + rt * 8 * 64 * PRE_ROW + lrow;
  const __bf16* a2 = x2img + rt * 8 * 64 * PRE_ROW + lrow;
  const __bf16* bt = wh6 + (long)(n0 / BN) * NKT * BN * PRE_ROW + tid * 8;  // this thread's first B piece of tile 0
  auto aptr = [&](int kt) {  // (kt is a compile-time constant in the unrolled loop)
    return kt < NH ? ah + (long)kt * 64 * PRE_ROW
                   : (kt < NH + 8 ? a0 : kt < NH + 16 ? a1 : a2) + (long)((kt - NH) % 8) * 64 * PRE_ROW;
  };
  u32x4 A[3][3], B[2][BP];  // A: tiles kt, kt+1, kt+2 (3 planes each); B: pieces of the tiles one / two ahead
  auto load_a = [&](u32x4 (&a)[3], int kt) {
    const __bf16* p = aptr(kt);
#pragma unroll
    for (int s = 0; s < 3; ++s) a[s] = *reinterpret_cast<const u32x4*>(p + s * BK6);
  };
  auto load_b = [&](u32x4 (&b)[BP], int kt) {
#pragma unroll
    for (int u = 0; u < BP; ++u) b[u] = *reinterpret_cast<const u32x4*>(bt + ((long)kt * BN * PRE_ROW + u * 256 * 8));
  };
  auto store_b = [&](const u32x4 (&b)[BP], __bf16* st, int u) {
    const int i = tid + 256 * u;
    *reinterpret_cast<u32x4*>(st + (i / (PRE_ROW / 8)) * LROW6 + (i % (PRE_ROW / 8)) * 8) = b[u];
  };
  // B fragments of a stage, read at the start of the tile's step
  auto read_b = [&](bf16x8 (&f)[TN][3], const __bf16* st, int j) {
    const __bf16* pb = st + (16 * j + l16) * LROW6 + 8 * q;
#pragma unroll
    for (int s = 0; s < 3; ++s) f[j][s] = *reinterpret_cast<const bf16x8*>(pb + s * BK6);
  };
  f32x4 acc[1][TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) acc[0][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bpre[TN];  // the epilogue's bias values, loaded ahead of the main loop
#pragma unroll
  for (int j = 0; j < TN; ++j) bpre[j] = d.bh[n0 + 16 * j + l16];
  load_a(A[0], 0);
  load_b(B[0], 0);
  load_a(A[1], 1);
  load_b(B[1], 1);
#pragma unroll
  for (int u = 0; u < BP; ++u) store_b(B[0], smem, u);
  __syncthreads();
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    // B pieces in flight: tile kt+2 into set kt % 2 (tile kt+1, set (kt+1) % 2, is stored this step)
    if (kt + NS < NKT) load_b(B[(kt + NS) % 2], kt + NS);
    if (kt + 2 < NKT) load_a(A[(kt + 2) % 3], kt + 2);
    __builtin_amdgcn_sched_barrier(0);  // the loads first
    const int ts = kt + 1;  // the tile this step stages
    __bf16* stg = smem + (ts % NS) * STG;
    bf16x8 f[TN][3];
#pragma unroll
    for (int j = 0; j < TN; ++j) read_b(f, smem + (kt % NS) * STG, j);
    // gemm6_core.h's six products per accumulator in its order (a2b0, a1b1, a0b2, a1b0, a0b1, a0b0), as six passes over
    // the four accumulators; between the passes the staged tile's pieces
#pragma unroll
    for (int u = 0; u < 6; ++u) {
      const int as = u == 0 ? 2 : (u == 1 || u == 3) ? 1 : 0, bs = u == 0 || u == 3 || u == 5 ? 0 : u == 2 ? 2 : 1;
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, A[kt % 3][as]), f[j][bs],
                                                            acc[0][j], 0, 0, 0);
      if (ts < NKT && u < BP) store_b(B[ts % 2], stg, u);
    }
    __syncthreads();
  }
  SD_TR(2)
  ep_bias_part<BM, BN, 64, KH_PW>(acc, d.bh, hp, d.D, ph, M, m0, n0, nullptr, bpre);
  SD_TR_END(tr.p, tr.slot)
}

// k_lin6 on register A operands: the step's three (N, D) x (D, U) deter contractions as one (N, D) x
// (D, nprob * U) product over the problems' concatenated columns, in 64-row x (16 NSUB)-column tiles of 512 threads
// whose K range is split between the two halves of the workgroup (waves 0-3: k tiles 0 .. NKH - 1, waves 4-7:
// NKH .. 2 NKH - 1). Each half has k_hid_areg's structure: wave w's 16 rows loaded per lane from the deter image into
// register fragments two tiles ahead, the half's weight tile through its own double-buffered LDS stage, 6 NSUB MFMAs
// per A fragment set (k_lin6's 32 x 32 tiles have 6, too few to pay for fragment-shaped loads, profiles/r05za); then
// the halves exchange half of their accumulators through LDS and each runs k_lin6's epilogue on two of every lane's
// four rows. NSUB = 3 (48 columns: 16 x 16 =
// 256 workgroups for three problems, one per CU) or 4 (the two-problem launch). The weight images are in 16-column
// tiles (k_presplit6<16>), so a tile's three or four 16-column pieces may come from different problems; the 16-column
// row-partial groups never straddle two. The halves' sums are added at the end, so the outputs agree with k_lin6's
// one pass to fp32 rounding, not bit for bit (test_lin6_areg_matches_lin6); NSUB 3 and 4 give the same values.
template <int NKH, int NSUB>
__global__ __launch_bounds__(512, 2) void k_lin6_areg(const __bf16* aimg, int K, const __bf16* w0, const __bf16* w1,
                                                      const __bf16* w2, LinProb p0, LinProb p1, LinProb p2, int U,
                                                      int M, Tr tr) {
  SD_TR_BEGIN
  constexpr int KQ = 2;  // K parts per workgroup (256 threads each)
  constexpr int BM = 64, BN = 16 * NSUB, NS = 2, PPS = 16 * PRE_ROW / 8;  // PPS: 16-B pieces per 16-column piece
  constexpr int STG = BN * LROW6, BP = (NSUB * PPS + 255) / 256;
  static_assert(KQ * BM * (BN + 4) * 4 <= KQ * NS * STG * 2, "reduce buffer within the stages");
  __bf16* smem = sd_smem6<KQ * NS * STG>();
  int tx = blockIdx.x, ty = blockIdx.y, tz = 0;
  xcd_tile(tx, ty, tz);
  const int c0 = tx * BN, m0 = ty * BM, nkt = K / BK6;
  const int tid = threadIdx.x, half = tid >> 8, htid = tid & 255, lane = tid & 63, wave = (tid >> 6) & 3;  // half: K part
  const int l16 = lane & 15, q = lane >> 4;
  SD_TR(1)
  const int kt0 = half * NKH;
  const __bf16* ah = aimg + ((long)(m0 / 64) * nkt + kt0) * 64 * PRE_ROW + (long)(16 * wave + l16) * PRE_ROW + 8 * q;
  // this thread's B pieces: piece i = htid + 256 u of the tile, 16-column piece i / PPS (column c0 + 16 (i / PPS))
  const __bf16* bt[BP];
  int boff[BP];
#pragma unroll
  for (int u = 0; u < BP; ++u) {
    const int i = htid + 256 * u, sp = i < NSUB * PPS ? i / PPS : 0, c = c0 + 16 * sp, pz = c / U;
    const __bf16* img = pz == 0 ? w0 : (pz == 1 ? w1 : w2);
    bt[u] = img + (((long)((c % U) / 16) * nkt + kt0) * 16) * PRE_ROW + (i % PPS) * 8;
    boff[u] = (16 * sp + (i % PPS) / (PRE_ROW / 8)) * LROW6 + (i % (PRE_ROW / 8)) * 8;
  }
  auto live = [&](int u) { return 256 * (u + 1) <= NSUB * PPS || htid + 256 * u < NSUB * PPS; };
  __bf16* hs = smem + half * NS * STG;
  u32x4 A[3][3], B[2][BP];
  auto load_a = [&](u32x4 (&a)[3], int kt) {
    const __bf16* pa = ah + (long)kt * 64 * PRE_ROW;
#pragma unroll
    for (int s = 0; s < 3; ++s) a[s] = *reinterpret_cast<const u32x4*>(pa + s * BK6);
  };
  auto load_b = [&](u32x4 (&b)[BP], int kt) {
#pragma unroll
    for (int u = 0; u < BP; ++u)
      if (live(u)) b[u] = *reinterpret_cast<const u32x4*>(bt[u] + (long)kt * 16 * PRE_ROW);
  };
  auto store_b = [&](const u32x4 (&b)[BP], __bf16* st, int u) {
    if (live(u)) *reinterpret_cast<u32x4*>(st + boff[u]) = b[u];
  };
  bf16x8 f[NSUB][3];
  f32x4 acc[NSUB];
#pragma unroll
  for (int j = 0; j < NSUB; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the epilogue's bias values, loaded ahead of the main loop (a problem without a bias reads a valid dummy address,
  // unconditionally, and takes 0)
  float bpre[NSUB];
#pragma unroll
  for (int j = 0; j < NSUB; ++j) {
    const int c = c0 + 16 * j, pz = c / U;
    const float* bp = pz == 0 ? p0.bias : (pz == 1 ? p1.bias : p2.bias);
    const float bl = (bp ? bp : reinterpret_cast<const float*>(aimg))[c % U + l16];
    bpre[j] = bp ? bl : 0.f;
  }
  load_a(A[0], 0);
  load_b(B[0], 0);
  load_a(A[1], 1);
  load_b(B[1], 1);
#pragma unroll
  for (int u = 0; u < BP; ++u) store_b(B[0], hs, u);
  __syncthreads();
#pragma unroll
  for (int kt = 0; kt < NKH; ++kt) {
    if (kt + NS < NKH) load_b(B[(kt + NS) % 2], kt + NS);
    if (kt + 2 < NKH) load_a(A[(kt + 2) % 3], kt + 2);
    __builtin_amdgcn_sched_barrier(0);  // the loads first
    const int ts = kt + 1;  // the tile this step stages
    __bf16* stg = hs + (ts % NS) * STG;
#pragma unroll
    for (int j = 0; j < NSUB; ++j) {
      const __bf16* pb = hs + (kt % NS) * STG + (16 * j + l16) * LROW6 + 8 * q;
#pragma unroll
      for (int s = 0; s < 3; ++s) f[j][s] = *reinterpret_cast<const bf16x8*>(pb + s * BK6);
    }
    // gemm6_core.h's six products per accumulator in its order, as six passes over the accumulators
#pragma unroll
    for (int u = 0; u < 6; ++u) {
      const int as = u == 0 ? 2 : (u == 1 || u == 3) ? 1 : 0, bs = u == 0 || u == 3 || u == 5 ? 0 : u == 2 ? 2 : 1;
#pragma unroll
      for (int j = 0; j < NSUB; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, A[kt % 3][as]), f[j][bs], acc[j],
                                                         0, 0, 0);
      if (ts < NKH && u < BP) store_b(B[ts % 2], stg, u);
    }
    __syncthreads();
  }
  SD_TR(2)
  // the K parts' sums meet through LDS (the stages are free after the loop's last barrier): part p finishes rows
  // r = p RPP .. of each lane's four, adding the KQ parts in index order (KQ = 2: a + b = b + a either way), so every
  // part runs the epilogue
  constexpr int LDR = BN + 4, RPP = 4 / KQ;
  float* red = reinterpret_cast<float*>(smem);
  const int rk = RPP * half;  // the rows this part keeps; it hands over the others
#pragma unroll
  for (int j = 0; j < NSUB; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r / RPP != half) red[((half * BM) + 16 * wave + 4 * q + r) * LDR + 16 * j + l16] = acc[j][r];
  __syncthreads();
  // ep_bias_part's arithmetic per 16-column piece of its problem: out = acc + bias (+ add), part = the piece's sum
  // of squares (one 16-column group)
#pragma unroll
  for (int j = 0; j < NSUB; ++j) {
    const int c = c0 + 16 * j, pz = c / U, n = c % U + l16;
    const LinProb& p = pz == 0 ? p0 : (pz == 1 ? p1 : p2);
    const float bv = bpre[j];
    float ss[RPP];
#pragma unroll
    for (int i = 0; i < RPP; ++i) {
      const int r = rk + i, m = m0 + 16 * wave + 4 * q + r, o = (16 * wave + 4 * q + r) * LDR + 16 * j + l16;
      float sum = half == 0 ? acc[j][r] : red[o];
#pragma unroll
      for (int pp = 1; pp < KQ; ++pp) sum += pp == half ? acc[j][r] : red[pp * BM * LDR + o];
      float v = sum + bv;
      if (p.add && m < M) v += p.add[(long)m * p.ldo + n];
      if (m < M) p.out[(long)m * p.ldo + n] = v;
      ss[i] = 0.f;
      ss[i] += v * v;
    }
#pragma unroll
    for (int i = 0; i < RPP; ++i) {
      const float sv = group_sum<16>(ss[i]);
      const int m = m0 + 16 * wave + 4 * q + rk + i;
      if (l16 == 0 && p.part && m < M) p.part[(long)((c % U) / 16) * M + m] = sv;
    }
  }
  SD_TR_END(tr.p, tr.slot)
}

// gates = BlockLinear(dyn_gru)(silu(rms(hp))) + bg; deter' = GRU (rssm.py:65-75) -> feats[t+1][:, SK:].
// Tile: 64 rows x (r | c | u) for 32 deter columns of block g (BN = 96). grid (D/32, M/64). B is _dyn_gru's
// once-per-imagination pre-split image (k_presplit6_gate), tile c0 / 32.
constexpr int KG_WAVES = 4;  // minimum waves per SIMD for k_gate's register allocation (its LDS admits 4 per CU)
__global__ __launch_bounds__(256, KG_WAVES) void k_gate(sd_imagine d, const float* hp, const float* ph, int nph,
                                              const float* hold, float* hnew, long ldf, const __bf16* wg6,
                                              __bf16* himg, Tr tr) {
  SD_TR_BEGIN
  constexpr int BM = 64, BN = 96;
  const int Dg = d.D / d.G;
  const int c0 = xcd_col(blockIdx.x, gridDim.x, Dg / 32) * 32, m0 = blockIdx.y * BM, g = c0 / Dg, j0 = c0 % Dg;
  __shared__ float rs[BM], red[256];
  wg_rstd<BM, 16>(ph, nph, d.N, m0, d.D, d.eps, rs, red);
  SD_TR(1)
  const ARms<BM> a0(hp + (long)g * Dg, d.D, d.nh + (long)g * Dg, rs, m0, d.N, Dg);
  const BPre6<BN> b0(wg6, c0 / 32, Dg / BK6, 0);
  // the GRU epilogue's operands (old deter, gate biases) loaded before the main loop, rows clamped: they arrive with
  // the first k tile instead of as a dependent round trip after the last
  const Lane L = lane_ids<BN, BN>();
  const float* bg = d.bg + (long)g * 3 * Dg;
  float hold_[2][4], bias_[2][3];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = 16 * j + L.l16, jj = j0 + c, col = c0 + c;
    bias_[j][0] = bg[jj];
    bias_[j][1] = bg[Dg + jj];
    bias_[j][2] = bg[2 * Dg + jj];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long m = m0 + L.wr * 16 + 4 * L.q + r;
      hold_[j][r] = hold[(m < d.N ? m : d.N - 1) * ldf + col];
    }
  }
  f32x4 acc[1][6];
  ARms<BM> la[KG_PF];
  BPre6<BN> lb[KG_PF];
#pragma unroll
  for (int u = 0; u < KG_PF; ++u) {
    la[u] = a0;
    lb[u] = b0;
  }
  gemm6_mainloop_1s<BM, BN, 16, BN, KG_PF>(la, lb, 0, Dg, acc);
  SD_TR(2)
  float hv_[2][4] = {};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = c0 + 16 * j + L.l16;
    const float br = bias_[j][0], bc = bias_[j][1], bu = bias_[j][2];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long m = m0 + L.wr * 16 + 4 * L.q + r;
      if (m >= d.N) continue;
      const float ra = acc[0][j][r] + br, ca = acc[0][2 + j][r] + bc, ua = acc[0][4 + j][r] + bu;
      const float rs = sigmoidf_(ra);
      const float cc = tanhf(rs * ca);
      const float u = sigmoidf_(ua - 1.f);
      const float hv = u * cc + (1.f - u) * hold_[j][r];
      hnew[m * ldf + col] = hv;
      hv_[j][r] = hv;
    }
  }
  if (himg) {  // the 64 x 32 tile of the new deter is exactly one pre-split image tile: staged in LDS, split, written
    constexpr int STG = (BM + BN) * LROW6;
    float* T = reinterpret_cast<float*>(sd_smem6<STG>());  // the main loop's image, free now
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) T[(L.wr * 16 + 4 * L.q + r) * 36 + 16 * j + L.l16] = hv_[j][r];
    __syncthreads();
    const int row = threadIdx.x >> 2, c8 = (threadIdx.x & 3) * 8;
    if (m0 + row < d.N) {
      pre_store4(himg, m0 + row, c0 + c8, d.D, *reinterpret_cast<const f32x4*>(T + row * 36 + c8));
      pre_store4(himg, m0 + row, c0 + c8 + 4, d.D, *reinterpret_cast<const f32x4*>(T + row * 36 + c8 + 4));
    }
  }
  SD_TR_END(tr.p, tr.slot)
}

// prior logits = img_net_logit(silu(rms(x))) and the unimix one-hot ST sample -> feats[t+1][:, :SK], on RTile<16>:
// grid (SK / 64, M / 16), 1024 threads (one sampler element per thread: row i / 64, column i % 64, teams of KD lanes);
// the noise drawn / read before the contraction
template <int KD>
__global__ __launch_bounds__(1024, 8) void k_prior_rw(sd_imagine d, const float* X, const float* nw,
                                                      const float* part_in, int np, float* snew, long ldf, int t,
                                                      Tr tr) {
  SD_TR_BEGIN
  using RT = RTile<16>;
  __shared__ __attribute__((aligned(16))) float P[16 * RT::LDP];
  __shared__ float red[16 * 4 * 64];
  __shared__ float T[16 * 65];
  const int tid = threadIdx.x, n0 = blockIdx.x * 64, m0 = blockIdx.y * 16, S = d.SK / KD;
  RT rt;
  rt.load_w(d.Wl, RT::U, n0);
  // sampler elements i = tid + NT e per thread: one. Written as loops over e: hipcc schedules the kernel's loads
  // differently around the same statements written without them, and this is the form that was measured
  constexpr int NT = 1024, PE = 1024 / NT;
  float gn[PE], blv[PE];
#pragma unroll
  for (int e = 0; e < PE; ++e) {
    const int i = tid + NT * e, rl = i >> 6, c = i & 63;
    const long m = m0 + rl, mc = m < d.N ? m : d.N - 1;
    // drawn ahead (sd_imagine_noise, the same values): one unconditional load (address select), else drawn below
    gn[e] = *(d.noise_img ? d.noise_img + ((long)t * d.N + mc) * d.SK + n0 + c : d.bl + n0 + c);
    blv[e] = d.bl[n0 + c];
  }
  RT::stage(P, X, RT::U, nw, part_in, np, d.N, m0, d.eps);  // (its wait covers the noise loads issued before)
  if (!d.noise_img) {
    const uint64_t seed = d.seed + (d.seed_ptr ? *d.seed_ptr : 0ull);
#pragma unroll
    for (int e = 0; e < PE; ++e) {
      const int i = tid + NT * e, rl = i >> 6, c = i & 63, lt = c % KD;
      gn[e] = sd_gumbel(seed, (uint32_t)d.stream_img, (uint32_t)t,
                        (uint64_t)((m0 + rl + d.row_offset) * S + (n0 + c) / KD) * KD + lt);
    }
  }
  __syncthreads();
  SD_TR(1)
  rt.mma(P);
  rt.reduce(red, T);
  SD_TR(2)
#pragma unroll
  for (int e = 0; e < PE; ++e) {
    const int i = tid + NT * e, rl = i >> 6, c = i & 63, lt = c % KD;
    const long m = m0 + rl;
    const float l = T[rl * 65 + c] + blv[e];
    float p, pp, nl;
    unimix_forward<KD>(l, true, KD, d.unimix, p, pp, nl);
    float ys;
    int idx;
    st_soft<KD>(nl, gn[e], true, ys, idx, lt);
    if (m < d.N) snew[m * ldf + n0 + c] = ((lt == idx ? 1.f : 0.f) - ys) + ys;
  }
  SD_TR_END(tr.p, tr.slot)
}

// actor output layer + action sample (bounded normal: loc = tanh, scale in [min_std, max_std]; or unimix one-hot),
// action_norm, and the action branch of the next Deter step: x2 = silu(rms(_dyn_in2(a_n))) (rssm.py:40-46).
// By rows: one wave per row, 4 rows per workgroup (N / 4 workgroups: 256 at the bench shape, where the former 16-row
// MFMA tiles gave 64). The chain has no workgroup barrier: the row's RMSNorm from the producer's partials, the actor
// output layer as fp32 dot products (4 columns per lane, one wave reduction per output), the action sample (bounded
// normal / unimix one-hot on lanes 0..15), action_norm, and x2 for the lane's 4 columns. Noise element (row, j) is
// counter (m + row_offset) * A + j of stream_act at step t, as sd_imagine_noise draws it.
// X0: also the next k_hid's x0 operand as a pre-split image, x0img = split(silu(rms(x0p) * n0)) (k_hid_areg; the
// row's rstd summed from k_lin6's partials in wg_rstd<64, 8>'s association, so the planes are those k_hid's own ARms
// loader would stage)
struct X0Img {
  const float* x0p;
  const float* px0;
  int npx0;
  __bf16* img;
};
template <int MO>  // >= the output logits (2A or A): 16 or 32
__global__ __launch_bounds__(256) void k_action_rows(sd_imagine d, const float* X, const float* nw,
                                                     const float* part_in, int np, float* act, float* x2, int t,
                                                     int want_x2, __bf16* x2img, X0Img x0i, Tr tr) {
  SD_TR_BEGIN
  constexpr int U = 256, MA = 16;  // <= 16 actions
  __shared__ float w2s[U * MA];    // _dyn_in2's weight (U, A), staged coalesced while the logits chain runs
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long m = (long)blockIdx.x * 4 + wave;
  const int A = d.A, NO = d.act_discrete ? A : 2 * A, M = d.N;
  const bool live = m < M;
  const uint64_t seed = d.seed + (d.seed_ptr ? *d.seed_ptr : 0ull);
  // operand loads first, every one unconditional (clamped row / partial / output-row indices; values past them are
  // masked where used — a "cond ? load : 0" made hipcc branch around each load and drain the queue at the join): the
  // row's partials, its 4 columns, the norm weight, the output layer's rows, then _dyn_in2's weight (into registers,
  // stored to LDS after the logits, so the logits chain waits on none of it) and the drawn-ahead action noise
  const long mc = live ? m : M - 1;
  const float pv_ = part_in[(long)(lane < np ? lane : np - 1) * M + mc];
  const f32x4 xv = ld4(X + mc * U + 4 * lane);
  const f32x4 wn = ld4(nw + 4 * lane);
  f32x4 wo[MO];
#pragma unroll
  for (int o = 0; o < MO; ++o) wo[o] = ld4(d.Wao + (long)(o < NO ? o : NO - 1) * U + 4 * lane);
  const float bo_ = d.bao[lane < NO ? lane : NO - 1];
  const bool x2w = want_x2 != 0;
  constexpr int W2R = U * MA / 256;
  float w2r[W2R];
#pragma unroll
  for (int k = 0; k < W2R; ++k) {
    const int i = threadIdx.x + 256 * k;
    w2r[k] = d.W2[i < U * A ? i : U * A - 1];
  }
  const f32x4 b2 = ld4(d.b2 + 4 * lane), n2 = ld4(d.n2 + 4 * lane);
  const bool x0w = x0i.img != nullptr && want_x2 != 0;  // (uniform over the launch)
  const float* x0src = x0w ? x0i.x0p : X;  // (a valid row either way: the loads stay unconditional)
  const f32x4 x0v = ld4(x0src + mc * U + 4 * lane), n0v = ld4((x0w ? d.n0 : nw) + 4 * lane);
  const int np0 = x0w ? x0i.npx0 : np;
  const float p0_ = (x0w ? x0i.px0 : part_in)[(long)(lane < np0 ? lane : np0 - 1) * M + mc];
  const int la = lane < A ? lane : A - 1;
  float nz = *(d.noise_act ? d.noise_act + ((long)t * M + mc) * A + la : d.b2);
  if (!d.noise_act) {  // drawn here (the same counter-based values as the drawn-ahead noise)
    nz = 0.f;
    if (d.act_discrete) {
      if (lane < A) nz = sd_gumbel(seed, (uint32_t)d.stream_act, (uint32_t)t, (uint64_t)(m + d.row_offset) * A + lane);
    } else if (lane < A) {
      nz = sd_normal(seed, (uint32_t)d.stream_act, (uint32_t)t, (uint64_t)(m + d.row_offset) * A + lane);
    }
  } else if (!(live && lane < A)) {
    nz = 0.f;
  }
  const float pv = (live && lane < np) ? pv_ : 0.f, bo = lane < NO ? bo_ : 0.f;
  const float rs = rsqrtf(wave_sum(pv) / (float)U + d.eps);
  SD_TR(1)
  f32x4 y;
#pragma unroll
  for (int j = 0; j < 4; ++j) y[j] = siluf_(xv[j] * rs * wn[j]);
  // the NO dot products, reduced over the wave stage by stage (independent shuffles in flight together)
  float pd[MO];
#pragma unroll
  for (int o = 0; o < MO; ++o) {
    float v = y[0] * wo[o][0];
    v = fmaf(y[1], wo[o][1], v);
    v = fmaf(y[2], wo[o][2], v);
    pd[o] = fmaf(y[3], wo[o][3], v);
  }
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1)
#pragma unroll
    for (int o = 0; o < MO; ++o)
      if (o < NO) pd[o] += __shfl_xor(pd[o], sh, 64);
  float lo = 0.f;  // lane o < NO: logit o (lanes past NO: 0, as with the former zero rows)
#pragma unroll
  for (int o = 0; o < MO; ++o)
    if (lane == o && o < NO) lo = pd[o];
  lo += bo;
  SD_TR(2)
  float a = 0.f;  // lane j < A: action element j
  if (d.act_discrete) {
    const bool on = lane < A;
    float p, pp, nl;
    unimix_forward<16>(lo, on, A, d.act_unimix, p, pp, nl);  // lanes 0..15 form the team
    float ys;
    int idx;
    st_soft<16>(nl, nz, on, ys, idx, lane & 15);
    if (on) a = ((lane == idx ? 1.f : 0.f) - ys) + ys;
  } else {
    const float ls = __shfl(lo, lane + A, 64);  // the scale logit of element lane
    if (lane < A) {
      const float loc = tanhf(lo);
      const float sc = (d.max_std - d.min_std) * sigmoidf_(ls + 2.f) + d.min_std;
      a = loc + nz * sc;
    }
  }
  if (live && lane < A) act[m * A + lane] = a;
  if (x0w) {  // wg_rstd<64, 8>: partial group g = p % 4 sums p = g, g + 4, ... in order, then the groups in order
    const float pp = lane < np0 ? p0_ : 0.f;
    float tt = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float sg = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) sg += __shfl(pp, g + 4 * k, 64);
      tt += sg;
    }
    const float r0 = rsqrtf(tt / (float)U + d.eps);
    f32x4 y0;
#pragma unroll
    for (int j = 0; j < 4; ++j) y0[j] = siluf_(x0v[j] * r0 * n0v[j]);
    if (live) pre_store4(x0i.img, m, 4 * lane, U, y0);
  }
  if (!x2w) {  // (uniform over the launch)
    SD_TR_END(tr.p, tr.slot)
    return;
  }
#pragma unroll
  for (int k = 0; k < W2R; ++k) {
    const int i = threadIdx.x + 256 * k;
    if (i < U * A) w2s[i] = w2r[k];
  }
  __syncthreads();  // w2s staged
  const float an = a / fmaxf(fabsf(a), 1.f);
  float anj[MA];
#pragma unroll
  for (int j = 0; j < MA; ++j) anj[j] = __shfl(an, j, 64);
  // x2p[4 lane + e] = b2 + sum_j a_n[j] W2[4 lane + e][j], b2 first, then j = 0, 1, ...
  f32x4 xp = b2;
#pragma unroll
  for (int j = 0; j < MA; ++j)
    if (j < A) {
#pragma unroll
      for (int e = 0; e < 4; ++e) xp[e] += anj[j] * w2s[(4 * lane + e) * A + j];
    }
  const float r2 = rsqrtf(wave_sum(xp[0] * xp[0] + xp[1] * xp[1] + xp[2] * xp[2] + xp[3] * xp[3]) / (float)U + d.eps);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = siluf_(xp[e] * r2 * n2[e]);
  if (live) {
    *reinterpret_cast<f32x4*>(x2 + m * U + 4 * lane) = o;
    if (x2img) pre_store4(x2img, m, 4 * lane, U, o);
  }
  SD_TR_END(tr.p, tr.slot)
}

// noise[t][m][k] = sd_gumbel(seed, stream_img, t, (m + row_offset) * SK + k) for t < H1 - 1: one thread per 4
// consecutive k, which share one Philox block (sd_gumbel's word idx & 3), one float4 store
__global__ __launch_bounds__(256) void k_imag_noise(sd_imagine d, float* noise, float* noise_act) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x, per_t = (long)d.N * d.SK / 4;
  const long nact = noise_act ? (long)d.H1 * d.N * d.A : 0;
  if (i < nact) {  // the action noise: the value k_action_rows would draw for (step, row, element)
    const int t = (int)(i / ((long)d.N * d.A));
    const long r = i - (long)t * d.N * d.A, m = r / d.A;
    const int j = (int)(r % d.A);
    const uint64_t seed = d.seed + (d.seed_ptr ? *d.seed_ptr : 0ull);
    const uint64_t e = (uint64_t)(m + d.row_offset) * d.A + j;
    noise_act[i] = d.act_discrete ? sd_gumbel(seed, (uint32_t)d.stream_act, (uint32_t)t, e)
                                  : sd_normal(seed, (uint32_t)d.stream_act, (uint32_t)t, e);
  }
  if (i >= (long)(d.H1 - 1) * per_t) return;
  const int t = (int)(i / per_t);
  const long r = i - (long)t * per_t, m = r / (d.SK / 4), k = 4 * (r % (d.SK / 4));
  const uint64_t seed = d.seed + (d.seed_ptr ? *d.seed_ptr : 0ull);
  const uint64_t q = ((uint64_t)(m + d.row_offset) * d.SK + k) >> 2;
  const sd_u32x4 w = sd_philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)t, (uint32_t)d.stream_img,
                                      (uint32_t)seed, (uint32_t)(seed >> 32));
  const f32x4 g{(float)(-log(-log(sd_u01(w.x)))), (float)(-log(-log(sd_u01(w.y)))),
                (float)(-log(-log(sd_u01(w.z)))), (float)(-log(-log(sd_u01(w.w))))};
  *reinterpret_cast<f32x4*>(noise + 4 * i) = g;
}

// ------------------------------------------------------------------------------------------- host side
struct IWork {
  float *a[2], *pa[2], *ad, *x0p, *px0, *x1p, *px1, *x2, *hp, *ph, *i[2], *pi[2];
  __bf16 *wh6, *wg6;  // pre-split _dyn_hid / _dyn_gru weights (BPre6 images, 3 bf16 per element)
  float *waT, *w1T;   // actor layer 0's stoch columns and _dyn_in1, transposed (SK, U) for k_onehot_lin
  __bf16 *h6, *x16, *x26;  // pre-split activation images: deter, silu(rms(x1p)), x2; rows padded to 64
  __bf16* x06;             // and silu(rms(x0p)) for k_hid_areg
  __bf16 *wi6, *w06, *wad6;  // pre-split img_net_0 / _dyn_in0 / actor layer 0 (deter columns) weights
  long total;
};
long al64(long n) { return (n + 63) / 64 * 64; }
IWork iwork(const sd_imagine& d, float* base) {
  IWork w;
  long o = 0;
  auto take = [&](long n) { float* p = base ? base + o : nullptr; o += al64(n); return p; };
  const long NU = (long)d.N * d.U, NP = (long)d.N * (d.U / 16);  // up to 16-column row partials
  for (int k = 0; k < 2; ++k) { w.a[k] = take(NU); w.pa[k] = take(NP); }
  w.ad = take(NU);
  w.x0p = take(NU); w.px0 = take(NP);
  w.x1p = take(NU); w.px1 = take(NP);
  w.x2 = take(NU);
  w.hp = take((long)d.N * d.D);
  w.ph = take((long)d.N * (d.D / 32));
  for (int k = 0; k < 2; ++k) { w.i[k] = take(NU); w.pi[k] = take(NP); }
  const long Ig = d.D / d.G + 3L * d.U;
  w.wh6 = reinterpret_cast<__bf16*>(take((long)d.D * Ig * 3 / 2));
  w.wg6 = reinterpret_cast<__bf16*>(take((long)3 * d.D * (d.D / d.G) * 3 / 2));
  w.waT = take((long)d.SK * d.U);
  w.w1T = take((long)d.SK * d.U);
  const long rows = (d.N + 63L) / 64 * 64;
  w.h6 = reinterpret_cast<__bf16*>(take(rows * d.D * 3 / 2));
  w.x16 = reinterpret_cast<__bf16*>(take(rows * d.U * 3 / 2));
  w.x26 = reinterpret_cast<__bf16*>(take(rows * d.U * 3 / 2));
  w.x06 = reinterpret_cast<__bf16*>(take(rows * d.U * 3 / 2));
  w.wi6 = reinterpret_cast<__bf16*>(take((long)d.U * d.D * 3 / 2));
  w.w06 = reinterpret_cast<__bf16*>(take((long)d.U * d.D * 3 / 2));
  w.wad6 = reinterpret_cast<__bf16*>(take((long)d.U * d.D * 3 / 2));
  w.total = o;
  return w;
}

// The shapes every launch of sd_imagine_run is tiled for (DESIGN.md § 2.1 lists which kernel needs which):
//   Dg = D / G a multiple of 64: k_hid / k_hid_areg take 64-column tiles of hp and read the block of a tile as
//     n0 / Dg, so a tile may not straddle two blocks of the block-diagonal weight (and Dg / 64 tiles per block > 0);
//     it covers k_gate's 32-column tiles, the 32-deep k tiles of Dg and D, and the D / 64 row partials of hp;
//   SK a multiple of 64 (k_prior_rw's 64-column workgroups, whole teams of Kd = 16 / 32 lanes; 32-deep k tiles of the
//     dense _dyn_in1 / actor layer 0 contraction when S > 64);
//   U = 256 (one wave per row at 4 columns a lane, 16 row partials of 16 columns);
//   at most 32 actor output logits (k_action_rows<32>) and 16 actions (its _dyn_in2 stage).
int ishape(const sd_imagine* d) {
  if (d->N < 1 || d->H1 < 1 || d->U != 256 || d->G < 1 || d->D < 1 || d->D % d->G || d->D > 4096) return SD_ESHAPE;
  const int Dg = d->D / d->G;
  if (Dg % 64 || d->SK < 64 || d->SK % 64 || (d->Kd != 16 && d->Kd != 32)) return SD_ESHAPE;
  if (d->A < 1 || (d->act_discrete ? d->A > 16 : 2 * d->A > 32)) return SD_ESHAPE;
  if (d->actor_layers < 1 || d->actor_layers > 4 || d->img_layers < 1 || d->img_layers > 4) return SD_ESHAPE;
  return SD_OK;
}

int icheck(const sd_imagine* d) {
  if (!d || !d->feats || !d->actions || !d->work) return SD_EARG;
  const int rc = ishape(d);
  if (rc) return rc;
  if (d->t_begin < 0 || d->t_begin >= (d->t_end > 0 ? d->t_end : d->H1) || d->t_end > d->H1) return SD_EARG;
  return SD_OK;
}

}  // namespace

extern "C" int sd_imagine_noise(const sd_imagine* dp, float* noise, float* noise_act, sd_stream stream_) {
  if (!dp) return SD_EARG;
  sd_imagine dc = *dp;  // (feats / actions need not exist yet: the noise reads neither)
  if (!dc.feats) dc.feats = noise;
  if (!dc.actions) dc.actions = noise;
  const int rc = icheck(&dc);
  if (rc) return rc;
  if (!noise || ((uintptr_t)noise & 15)) return SD_EARG;
  long n = (long)(dp->H1 - 1) * dp->N * dp->SK / 4;
  if (noise_act) n = n > (long)dp->H1 * dp->N * dp->A ? n : (long)dp->H1 * dp->N * dp->A;
  if (n <= 0) return SD_OK;
  k_imag_noise<<<(int)((n + 255) / 256), 256, 0, (hipStream_t)stream_>>>(*dp, noise, noise_act);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_imagine_work_floats(const sd_imagine* d) {
  if (!d) return SD_EARG;
  const int rc = ishape(d);  // the shape gate, before any pointer exists: an unsupported shape gets no workspace
  if (rc) return rc;
  return (int)iwork(*d, nullptr).total;
}

// Which kernels one entry call launches. The runtime knobs are read here, once per call (tests toggle them in-process
// between calls), so every launch of a call — and the tile width of its weight images, which lareg decides — agrees.
struct IPlan {
  // k_hid reads deter / x1 / x2 from pre-split images, which every producer then writes (k_gate, k_onehot_lin,
  // k_action_rows); SDHIP_KH_NOAPRE set: the in-loader split, for tests comparing the two — bit-identical
  bool apre;
  // k_hid on register A operands (k_hid_areg) at the block widths it is built for (Dg = 256 / 512): its k tiles, else
  // 0; SDHIP_KH_NOAREG set: k_hid<true>, for A/B and the bit-identity test
  int areg_nkt;
  // the deter contractions on pre-split operands (k_lin6): A the deter image (apre), B the weights split once per
  // imagination; SDHIP_KL_NOPRE set: the fp32 k_lin, for A/B and tests
  bool lpre;
  // k_lin6_areg where it is built (D = 2048 / 4096: two halves of 32 / 64 k tiles), on weight images in 16-column
  // tiles (KL3_BN for k_lin6); SDHIP_KL_NOAREG set: k_lin6 (A/B, and the agreement test)
  bool lareg;
  // k_lin6_areg's three-problem launch on 48-column tiles; SDHIP_KL_NSUB4 set: 64-column tiles
  bool n3;
};
static IPlan iplan(const sd_imagine& d) {
  static_assert(256 % KL3_BN == 0 && KH_BM == 64, "k_lin6's column tiles; the images' 64-row tiles");
  IPlan p;
  const int nkt = (d.D / d.G + 3 * d.U) / BK6;
  p.apre = d.SK / d.Kd <= 64 && !getenv("SDHIP_KH_NOAPRE");
  p.areg_nkt = (p.apre && (nkt == 32 || nkt == 40) && !getenv("SDHIP_KH_NOAREG")) ? nkt : 0;
  p.lpre = p.apre && !getenv("SDHIP_KL_NOPRE");
  p.lareg = p.lpre && (d.D == 64 * BK6 || d.D == 128 * BK6) && !getenv("SDHIP_KL_NOAREG");
  p.n3 = !getenv("SDHIP_KL_NSUB4");
  return p;
}

static void launch_hid_areg(const sd_imagine& d, const IWork& w, int nkt, Tr tr, hipStream_t st) {
  const dim3 grid(d.D / 64, sd_cdiv(d.N, 64));
  if (nkt == 32)
    k_hid_areg<32><<<grid, 256, 0, st>>>(d, w.hp, w.ph, w.wh6, w.h6, w.x06, w.x16, w.x26, tr);
  else
    k_hid_areg<40><<<grid, 256, 0, st>>>(d, w.hp, w.ph, w.wh6, w.h6, w.x06, w.x16, w.x26, tr);
}
// one k_lin6 / k_lin6_areg launch over nprob (2 or 3) problems sharing A = the deter image
static void launch_lin6(const sd_imagine& d, const IPlan& pl, const IWork& w, const __bf16* wa, const __bf16* wb,
                        const __bf16* wc, const LinProb& pa, const LinProb& pb, const LinProb& pc, int nprob, Tr tr,
                        hipStream_t st) {
  if (!pl.lareg) {
    k_lin6<KL6_BM, KL3_BN><<<dim3(d.U / KL3_BN, sd_cdiv(d.N, KL6_BM), nprob), 256, 0, st>>>(w.h6, d.D, wa, wb, wc, pa,
                                                                                          pb, pc, d.N, tr);
    return;
  }
  const bool n3 = nprob == 3 && pl.n3;
  const dim3 grid(n3 ? 3 * d.U / 48 : nprob * d.U / 64, sd_cdiv(d.N, 64));
  // k tiles per half of the workgroup: D / 32 / 2
  if (d.D == 64 * BK6 && n3)
    k_lin6_areg<32, 3><<<grid, 512, 0, st>>>(w.h6, d.D, wa, wb, wc, pa, pb, pc, d.U, d.N, tr);
  else if (d.D == 64 * BK6)
    k_lin6_areg<32, 4><<<grid, 512, 0, st>>>(w.h6, d.D, wa, wb, wc, pa, pb, pc, d.U, d.N, tr);
  else if (n3)
    k_lin6_areg<64, 3><<<grid, 512, 0, st>>>(w.h6, d.D, wa, wb, wc, pa, pb, pc, d.U, d.N, tr);
  else
    k_lin6_areg<64, 4><<<grid, 512, 0, st>>>(w.h6, d.D, wa, wb, wc, pa, pb, pc, d.U, d.N, tr);
}

// One launch of step t's k_lin / k_lin6 (img_net_0 + _dyn_in0 + actor layer 0's deter part: which = 0), k_hid (1) or
// k_gate (2), exactly as sd_imagine_run issues it (same descriptor and workspace; the launch recomputes the values that
// run already wrote, so it can be repeated): bench.py times the dominant kernel of the update this way.
extern "C" int sd_imagine_step_kernel(const sd_imagine* dp, int which, int t, sd_stream stream_) {
  int rc = icheck(dp);
  if (rc) return rc;
  const sd_imagine& d = *dp;
  if (t < 0 || t >= d.H1 - 1 || which < 0 || which > 2) return SD_EARG;
  hipStream_t st = (hipStream_t)stream_;
  const IWork w = iwork(d, d.work);
  const IPlan pl = iplan(d);
  const int N = d.N, U = d.U, SK = d.SK, D = d.D, F = SK + D;
  const long NF = (long)N * F;
  const int npU = U / ROW_PW;
  auto feats = [&](int s) { return d.feats + s * NF; };
  if (which == 0) {
    LinProb pi{feats(t + 1) + SK, F, D, d.Wi[0], D, d.bi[0], w.i[0], U, w.pi[0], nullptr};
    LinProb px{feats(t + 1) + SK, F, D, d.W0, D, d.b0, w.x0p, U, w.px0, nullptr};
    LinProb pd{feats(t + 1) + SK, F, D, d.Wa[0] + SK, F, nullptr, w.ad, U, nullptr, nullptr};
    if (pl.lpre)  // the images the run built (the deter image holds its last step: the timing is the same)
      launch_lin6(d, pl, w, w.wi6, w.w06, w.wad6, pi, px, pd, 3, Tr{}, st);
    else
      k_lin<KL3_BM, KL3_BN><<<dim3(U / KL3_BN, sd_cdiv(N, KL3_BM), 3), 256, 0, st>>>(pi, px, pd, N, Tr{});
  } else if (which == 1 && pl.areg_nkt) {  // (the images the run built)
    launch_hid_areg(d, w, pl.areg_nkt, Tr{}, st);
  } else if (which == 1) {
    k_hid<false><<<dim3(D / 64, sd_cdiv(N, KH_BM)), 256, 0, st>>>(d, feats(t) + SK, F, w.x0p, w.x1p, w.px0, w.px1, npU,
                                                                 npU, w.x2, w.hp, w.ph, w.wh6, nullptr, nullptr,
                                                                 nullptr, Tr{});
  } else {
    // k_gate reads hold = feats(t) deter and writes feats(t + 1) deter: the same values again
    k_gate<<<dim3(D / 32, sd_cdiv(N, 64)), 256, 0, st>>>(d, w.hp, w.ph, D / KH_PW, feats(t) + SK, feats(t + 1) + SK, F,
                                                         w.wg6, nullptr, Tr{});
  }
  SD_LAUNCH_CHECK();
  return SD_OK;
}

// the weight-only setup of an imagination: pre-split images and transposed one-hot weights (sd_imagine_prep)
static int imagine_prep(const sd_imagine& d, const IPlan& pl, const IWork& w, hipStream_t st) {
  const int U = d.U, SK = d.SK, D = d.D, F = SK + D;
  const long Ig = D / d.G + 3L * U;  // _dyn_hid's and _dyn_gru's weights split into their bf16 planes
  k_presplit6<64><<<(int)sd_cdiv((long)D * Ig / 4, 256), 256, 0, st>>>(d.Wh, D, (int)Ig, w.wh6);
  SD_LAUNCH_CHECK();
  k_transpose_w<<<sd_cdiv((long)SK * U, 256), 256, 0, st>>>(d.Wa[0], F, U, SK, w.waT);  // the one-hot contractions'
  k_transpose_w<<<sd_cdiv((long)SK * U, 256), 256, 0, st>>>(d.W1, SK, U, SK, w.w1T);
  SD_LAUNCH_CHECK();
  k_presplit6_gate<<<(int)sd_cdiv((long)3 * D * (D / d.G) / 4, 256), 256, 0, st>>>(d.Wg, D, D / d.G, w.wg6);
  SD_LAUNCH_CHECK();
  if (pl.lpre) {  // the deter contractions' weights (img_net_0, _dyn_in0, actor layer 0's deter part)
    const float* Wa0d = d.Wa[0] + SK;
    const int gsz = (int)sd_cdiv((long)U * D / 4, 256);
    if (pl.lareg) {  // 16-column tiles for k_lin6_areg
      k_presplit6<16><<<gsz, 256, 0, st>>>(d.Wi[0], U, D, w.wi6, D);
      k_presplit6<16><<<gsz, 256, 0, st>>>(d.W0, U, D, w.w06, D);
      k_presplit6<16><<<gsz, 256, 0, st>>>(Wa0d, U, D, w.wad6, F);
    } else {
      k_presplit6<KL3_BN><<<gsz, 256, 0, st>>>(d.Wi[0], U, D, w.wi6, D);
      k_presplit6<KL3_BN><<<gsz, 256, 0, st>>>(d.W0, U, D, w.w06, D);
      k_presplit6<KL3_BN><<<gsz, 256, 0, st>>>(Wa0d, U, D, w.wad6, F);
    }
    SD_LAUNCH_CHECK();
  }
  return SD_OK;
}

extern "C" int sd_imagine_prep(const sd_imagine* dp, sd_stream stream_) {
  if (!dp) return SD_EARG;
  sd_imagine d = *dp;  // (feats / actions need not exist yet: the weight images read neither)
  if (!d.feats) d.feats = d.work;
  if (!d.actions) d.actions = d.work;
  const int rc = icheck(&d);
  if (rc) return rc;
  return imagine_prep(d, iplan(d), iwork(d, d.work), (hipStream_t)stream_);
}

extern "C" int sd_imagine_run(const sd_imagine* dp, sd_stream stream_) {
  int rc = icheck(dp);
  if (rc) return rc;
  const sd_imagine& d = *dp;
  hipStream_t st = (hipStream_t)stream_;
  const IWork w = iwork(d, d.work);
  const IPlan pl = iplan(d);
  const int N = d.N, U = d.U, SK = d.SK, D = d.D, F = SK + D;
  const long NF = (long)N * F;
  const int npU = U / ROW_PW;  // row partials per hidden row, whichever kernel wrote it
  auto feats = [&](int t) { return d.feats + t * NF; };
  // actor layer 0 on feat = [stoch, deter] is K-split: the deter part (no bias) runs in the launch that already
  // reads deter' (img_net_0 / _dyn_in0), the stoch part (+ bias + deter part, row partials) after the prior sample
  const float* Wa0d = d.Wa[0] + SK;  // (U, F) columns SK.. of the actor's first weight
  const int t_end = d.t_end > 0 ? d.t_end : d.H1;
  const bool apre = pl.apre;
  // the x0 image k_action_rows writes for k_hid_areg
  const X0Img x0i{w.x0p, w.px0, npU, pl.areg_nkt ? w.x06 : nullptr};
  if (d.t_begin == 0 && apre) {  // the start state's deter image
    k_presplit_rows<<<(int)sd_cdiv((long)N * D / 4, 256), 256, 0, st>>>(feats(0) + SK, F, N, D, w.h6);
    SD_LAUNCH_CHECK();
  }
  if (d.t_begin == 0 && !d.prepped) {
    const int e = imagine_prep(d, pl, w, st);
    if (e) return e;
  }
  if (d.t_begin == 0) {  // x0p(0) = h0 . W0^T + b0 and the deter part of actor layer 0 at t = 0
    LinProb p{feats(0) + SK, F, D, d.W0, D, d.b0, w.x0p, U, w.px0, nullptr};
    LinProb pd{feats(0) + SK, F, D, Wa0d, F, nullptr, w.ad, U, nullptr, nullptr};
    // the 3-problem launch's tile, so x0p's row partials have one width for every step
    if (pl.lpre)
      launch_lin6(d, pl, w, w.w06, w.wad6, w.wad6, p, pd, pd, 2, Tr{}, st);
    else
      k_lin<KL3_BM, KL3_BN><<<dim3(U / KL3_BN, sd_cdiv(N, KL3_BM), 2), 256, 0, st>>>(p, pd, pd, N, Tr{});
    SD_LAUNCH_CHECK();
  }
  for (int t = d.t_begin; t < t_end; ++t) {
    const bool last = t == d.H1 - 1;
    auto tr = [&](int k) { return Tr{d.trace, t * 16 + k}; };  // launch k of step t (measurement builds)
    // actor layer 0's output: the caller's per-step buffer when given (read again by the policy loss), else scratch
    float* a0 = d.actor_h0 ? d.actor_h0 + (long)t * N * U : w.a[0];
    {  // actor layer 0, stoch part (+ deter part); _dyn_in1 on stoch
      if (d.SK / d.Kd <= 64) {
        const OneHotProb oa{w.waT, d.ba[0], w.ad, a0, w.pa[0], nullptr, nullptr, 0.f},
            ox{w.w1T, d.b1, nullptr, w.x1p, w.px1, apre ? d.n1 : nullptr, apre ? w.x16 : nullptr, d.eps};
        k_onehot_lin<<<dim3(sd_cdiv(N, 4), last ? 1 : 2), 256, 0, st>>>(feats(t), F, SK, d.Kd, oa, ox, last ? 1 : 2, N,
                                                                       tr(0));
      } else {  // more categoricals than a wave has lanes: the dense contraction
        LinProb pa{feats(t), F, SK, d.Wa[0], F, d.ba[0], a0, U, w.pa[0], w.ad};
        LinProb px{feats(t), F, SK, d.W1, SK, d.b1, w.x1p, U, w.px1, nullptr};
        k_lin<32, KL2_BN><<<dim3(U / KL2_BN, sd_cdiv(N, 32), last ? 1 : 2), 256, 0, st>>>(pa, px, px, N, tr(0));
      }
      SD_LAUNCH_CHECK();
    }
    int cur = 0;
    for (int l = 1; l < d.actor_layers; ++l) {
      k_rmslin_rw<<<dim3(U / 64, sd_cdiv(N, 16)), 512, 0, st>>>(l == 1 ? a0 : w.a[cur], d.na[l - 1], w.pa[cur], npU,
                                                                 d.Wa[l], d.ba[l], w.a[cur ^ 1], w.pa[cur ^ 1], N,
                                                                 d.eps, tr(l));
      SD_LAUNCH_CHECK();
      cur ^= 1;
    }
    {
      const float* xa = d.actor_layers == 1 ? a0 : w.a[cur];
      float* acts = d.actions + (long)t * N * d.A;
      if ((d.act_discrete ? d.A : 2 * d.A) <= 16)
        k_action_rows<16><<<sd_cdiv(N, 4), 256, 0, st>>>(d, xa, d.na[d.actor_layers - 1], w.pa[cur], npU, acts, w.x2,
                                                         t, last ? 0 : 1, apre ? w.x26 : nullptr, x0i, tr(4));
      else
        k_action_rows<32><<<sd_cdiv(N, 4), 256, 0, st>>>(d, xa, d.na[d.actor_layers - 1], w.pa[cur], npU, acts, w.x2,
                                                         t, last ? 0 : 1, apre ? w.x26 : nullptr, x0i, tr(4));
    }
    SD_LAUNCH_CHECK();
    if (last) break;
    if (pl.areg_nkt)
      launch_hid_areg(d, w, pl.areg_nkt, tr(5), st);
    else if (apre)
      k_hid<true><<<dim3(D / 64, sd_cdiv(N, KH_BM)), 256, 0, st>>>(d, feats(t) + SK, F, w.x0p, w.x1p, w.px0, w.px1, npU,
                                                                  npU, w.x2, w.hp, w.ph, w.wh6, w.h6, w.x16, w.x26,
                                                                  tr(5));
    else
      k_hid<false><<<dim3(D / 64, sd_cdiv(N, KH_BM)), 256, 0, st>>>(d, feats(t) + SK, F, w.x0p, w.x1p, w.px0, w.px1,
                                                                   npU, npU, w.x2, w.hp, w.ph, w.wh6, nullptr, nullptr,
                                                                   nullptr, tr(5));
    SD_LAUNCH_CHECK();
    k_gate<<<dim3(D / 32, sd_cdiv(N, 64)), 256, 0, st>>>(d, w.hp, w.ph, D / KH_PW, feats(t) + SK, feats(t + 1) + SK, F,
                                                         w.wg6, apre ? w.h6 : nullptr, tr(6));
    SD_LAUNCH_CHECK();
    {  // img_net_0, the next step's _dyn_in0 and the deter part of its actor layer 0 share A = deter'
      LinProb pi{feats(t + 1) + SK, F, D, d.Wi[0], D, d.bi[0], w.i[0], U, w.pi[0], nullptr};
      LinProb px{feats(t + 1) + SK, F, D, d.W0, D, d.b0, w.x0p, U, w.px0, nullptr};
      LinProb pd{feats(t + 1) + SK, F, D, Wa0d, F, nullptr, w.ad, U, nullptr, nullptr};
      if (pl.lpre)
        launch_lin6(d, pl, w, w.wi6, w.w06, w.wad6, pi, px, pd, 3, tr(7), st);
      else
        k_lin<KL3_BM, KL3_BN><<<dim3(U / KL3_BN, sd_cdiv(N, KL3_BM), 3), 256, 0, st>>>(pi, px, pd, N, tr(7));
      SD_LAUNCH_CHECK();
    }
    int ci = 0;
    for (int l = 1; l < d.img_layers; ++l) {
      k_rmslin_rw<<<dim3(U / 64, sd_cdiv(N, 16)), 512, 0, st>>>(w.i[ci], d.ni[l - 1], w.pi[ci], npU, d.Wi[l], d.bi[l],
                                                                 w.i[ci ^ 1], w.pi[ci ^ 1], N, d.eps, tr(7 + l));
      SD_LAUNCH_CHECK();
      ci ^= 1;
    }
    const dim3 gpr(SK / 64, sd_cdiv(N, 16));
    if (d.Kd == 16)
      k_prior_rw<16><<<gpr, 1024, 0, st>>>(d, w.i[ci], d.ni[d.img_layers - 1], w.pi[ci], npU, feats(t + 1), F, t,
                                           tr(12));
    else
      k_prior_rw<32><<<gpr, 1024, 0, st>>>(d, w.i[ci], d.ni[d.img_layers - 1], w.pi[ci], npU, feats(t + 1), F, t,
                                           tr(12));
    SD_LAUNCH_CHECK();
  }
  return SD_OK;
}
