// Shared pieces of the fused RSSM step kernels (scan.hip) and the acting step built on them (policy.hip): the M = 16
// exact-fp32 MFMA contraction core, the prologue load helpers and the scratch layout.
#pragma once
#include "common.h"
#include "sdhip.h"

namespace {

constexpr int NW = 8;
constexpr int NTHR = 64 * NW;
constexpr int MR = 16;

SD_DEV f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
SD_DEV f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
SD_DEV void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
SD_DEV float dsilu(float z) {
  const float s = sigmoidf_(z);
  return s * (1.f + z * (1.f - s));
}

// ------------------------------------------------------------------------------------------- contraction core
// acc[t] += A[0:16, span] . W_t[n_t + 0:16, span]^T.  Wave w owns 16-deep k chunks; lane group q = lane>>4 supplies
// k = 16c + 4q .. +3 as one float4 and the MFMA consumes them in 4 steps (a permuted but consistent k order).
// A wave's chunks come in adjacent pairs (2w, 2w + 1, 2w + 16, 2w + 17, ...), so the two loads it issues back to back
// for a row cover one whole 128-B line (with single chunks c = w, w + 8, ... each 128-B line of a weight row was split
// between two waves' loads, issued at different times).
SD_DEV int core_chunk(int wave, int c) { return 2 * (wave + NW * (c >> 1)) + (c & 1); }
template <int NT, int CPW>
struct Core {
  static_assert(CPW % 2 == 0, "chunk pairs");
  f32x4 b[CPW][NT];
  f32x4 acc[NT];

  // Wt[t]: row (n_t + l16) of a k-contiguous weight matrix, at the span's first k (a valid row for EVERY lane: the
  // extra lanes of an 8-column tile point at a real row, their output columns are discarded). Chunks past nch load
  // chunk nch - 1 and are never multiplied: every load is unconditional (no branch around it, so hipcc has no join at
  // which to drain the queue — see "load helpers" below).
  SD_DEV void load_b(const float* const* Wt, int nch, int wave, int q) {
#pragma unroll
    for (int c = 0; c < CPW; ++c) {
      const int ch = core_chunk(wave, c), chc = ch < nch ? ch : nch - 1;
#pragma unroll
      for (int t = 0; t < NT; ++t) b[c][t] = ld4(Wt[t] + chc * 16 + 4 * q);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = zero4();
  }
  SD_DEV void mma(const f32x4& a, int c) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[c][t][j], acc[t], 0, 0, 0);
  }
  // A from an LDS panel with row stride lda (lda % 64 == 4)
  SD_DEV void run_lds(const float* P, int lda, int nch, int wave, int l16, int q) {
#pragma unroll
    for (int c = 0; c < CPW; ++c) {
      const int ch = core_chunk(wave, c);
      if (ch < nch) mma(ld4(P + l16 * lda + ch * 16 + 4 * q), c);
    }
  }
  // A straight from global memory; rows >= M read row M - 1 (their output rows are discarded by the callers), all
  // loads issued before the first MFMA
  SD_DEV void run_glb(const float* A, long lda, int M, int nch, int wave, int l16, int q) {
    f32x4 a[CPW];
    const int lr = l16 < M ? l16 : M - 1;
#pragma unroll
    for (int c = 0; c < CPW; ++c) {
      const int ch = core_chunk(wave, c), chc = ch < nch ? ch : nch - 1;
      a[c] = ld4(A + (long)lr * lda + chc * 16 + 4 * q);
    }
#pragma unroll
    for (int c = 0; c < CPW; ++c)
      if (core_chunk(wave, c) < nch) mma(a[c], c);
  }
  // sum the 8 waves' partial tiles into C (16 x 16NT, row-major) in LDS
  SD_DEV void reduce(float* red, float* C, int tid, int wave, int lane) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[((wave * NT + t) * 4 + r) * 64 + lane] = acc[t][r];
    __syncthreads();
    for (int i = tid; i < NT * 256; i += NTHR) {
      const int t = i >> 8, r = (i >> 6) & 3, ln = i & 63;
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) v += red[((w * NT + t) * 4 + r) * 64 + ln];
      C[(4 * (ln >> 4) + r) * (16 * NT) + t * 16 + (ln & 15)] = v;
    }
    __syncthreads();
  }
};

template <int NT>
constexpr int core_lds_floats() { return NW * NT * 256 + MR * 16 * NT; }

// row tile of a workgroup (grid z): batch rows rb .. rb + nr (d.row_tile rows, normalised on the host)
#define SD_ROW_TILE                                               \
  const int rb = (int)blockIdx.z * d.row_tile, nr = min(d.row_tile, d.B - rb); \
  (void)rb; (void)nr;

#define SD_THREAD_IDS                                      \
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6; \
  const int l16 = lane & 15, q = lane >> 4;                \
  (void)l16; (void)q;

// XCD-contiguous tiles: the dispatcher deals workgroup i to XCD i % 8, so tile (i % 8) * (n / 8) + i / 8 gives XCD x
// the n / 8 consecutive column tiles [x n / 8, (x + 1) n / 8) (with 16-column tiles over D = 2048: exactly block x).
// Each XCD then writes whole 128-B lines of every output row (two or four neighbouring tiles share a line), and the
// lines left dirty at the launch's end are not split between XCDs. Speed only: any tile order gives the same result
// (a tile count that is no multiple of 8 keeps the dispatch order).
SD_DEV int xcd_tile(int i, int n) { return n % 8 == 0 ? (i % 8) * (n / 8) + i / 8 : i; }

// ------------------------------------------------------------------------------------------- load helpers
// Prologues use 32 threads per row (16 rows): thread t32 owns the float4 columns c = 4*t32 + 128*i. Every load a
// launch needs is issued before the first use, and every load is UNCONDITIONAL: rows past the tile read a valid row
// (the callers clamp the row index; those rows' results are discarded), slabs past ks read slab ks - 1 (masked when
// summed). A predicated "cond ? load : 0" made hipcc branch around each load and drain the whole vector-memory queue
// (s_waitcnt vmcnt(0)) at the join, so the weight stream issued first and the prologue loads behind it became two
// dependent round trips (round 5: tools/isa_waits.py listed such drains in every scan kernel).
// Rows are exactly 128 * NI floats wide (every caller's width: U = 256, D/G, S*Kd are multiples of 128).
template <int NI>
SD_DEV void ld_row(f32x4 (&v)[NI], const float* rowp, int t32) {
#pragma unroll
  for (int i = 0; i < NI; ++i) v[i] = ld4(rowp + 4 * t32 + 128 * i);
}
// KS <= slab loads of ks split-K slabs (sum_slabs adds the first ks in fixed order, after the launch's other loads)
template <int NI, int KS>
SD_DEV void ld_slabs(f32x4 (&part)[KS][NI], const float* rowp, long sstride, int ks, int t32) {
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int sc = s < ks ? s : ks - 1;
#pragma unroll
    for (int i = 0; i < NI; ++i) part[s][i] = ld4(rowp + sc * sstride + 4 * t32 + 128 * i);
  }
}
template <int NI, int KS>
SD_DEV void sum_slabs(f32x4 (&v)[NI], const f32x4 (&part)[KS][NI], int ks) {
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    v[i] = part[0][i];
#pragma unroll
    for (int s = 1; s < KS; ++s)
      if (s < ks) v[i] += part[s][i];
  }
}
// per-tile row partials, row-major: part[row * tiles + i], i < tiles <= 128*NP (tiles % 4 == 0): a row's partials
// are one contiguous run, read as float4s by the row's 32 threads (the column-major layout cost 64 cache lines per
// wave instruction); entries past `tiles` re-read the last float4 and are masked in sum_parts
template <int NP>
SD_DEV void ld_parts(f32x4 (&v)[NP], const float* rowp, int tiles, int t32) {
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int i = 4 * (t32 + 32 * j);
    v[j] = *reinterpret_cast<const f32x4*>(rowp + (i < tiles ? i : tiles - 4));
  }
}
template <int NP>
SD_DEV float sum_parts(const f32x4 (&v)[NP], int tiles, int t32) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NP; ++j)
    if (4 * (t32 + 32 * j) < tiles) s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
  return group_sum<32>(s);
}
SD_DEV float sumsq4(f32x4 x) { return x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3]; }

// y = silu(x * r * w) (rows >= M -> 0), x already holds the row (incl. bias)
template <int NI>
SD_DEV float rms_silu_rows(f32x4 (&x)[NI], const f32x4 (&w)[NI], int N, float eps, bool rv, f32x4 (&y)[NI]) {
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NI; ++i) ss += sumsq4(x[i]);
  ss = group_sum<32>(ss);
  const float r = rsqrtf(ss / (float)N + eps);
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) y[i][j] = rv ? siluf_(x[i][j] * r * w[i][j]) : 0.f;
  return r;
}

template <int NI>
SD_DEV void st_row(float* rowp, const f32x4 (&v)[NI], int N, int t32) {
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int c = 4 * t32 + 128 * i;
    if (c < N) st4(rowp + c, v[i]);
  }
}

constexpr int KSM = 8;    // max split-K slabs of the D-wide step GEMMs (ks_d)
constexpr int LR_NG = 8;  // x1p slabs: the categorical groups per row of k_logit_rows (one slab each), summed by k_hid
static_assert(LR_NG == KSM && KSM == 8, "k_hid sums LR_NG x1p slabs and up to KSM x0p slabs: 8 each");
// categoricals per k_logit_rows workgroup: S / LR_NG (check() admits S = SK / Kd in {8, 16, 32, 64}, so >= 1)
constexpr int lr_cpg(int SK, int KD) { return SK / (LR_NG * KD); }
// Output columns per workgroup: 16 (one MFMA tile) in every kernel but k_gate, whose workgroups take 8 deter columns
// (GCW) with their r | c and u gate rows as two tiles (DESIGN.md § 4.2 has the measurements).
constexpr int GCW = 8;
long al64(long n) { return (n + 63) / 64 * 64; }
int row_tile_of(const sd_rssm_scan& d) { return d.row_tile > 0 ? d.row_tile : MR; }
int row_tiles(const sd_rssm_scan& d) { return (d.B + row_tile_of(d) - 1) / row_tile_of(d); }

}  // namespace

// ------------------------------------------------------------------------------------------- scratch layout
namespace sdscan {

struct Work {
  float *x0s, *x1s, *ops, *ssh, *dotp, *dxs, *dhin, *gq, *ch, *w1t;
  long total;
  // The acting step (policy.hip) runs the forward phases at T = 1 and fills the two operand slots the last step of
  // a scan leaves free with the two halves of actor layer 0 (all zero in a scan):
  //   step0: added to t in the posterior sample's Philox step counter;
  //   tail:  1 = phase 3's second k_slab problem is deter . tailW^T (row stride tail_ldw) into the x0s slabs, and
  //          k_logit_rows (its TAIL instantiation) gathers the sample's rows of w1t (then the transposed one-hot half)
  //          into the x1s slabs.
  int step0, tail;
  const float* tailW;
  long tail_ldw;
};

// one launch of forward step t's phase `which` (scan.hip: 0 x1p k_slab, 1 k_hid, 2 k_gate, 3 k_slab, 4 k_logit_rows)
int fwd_phase(const sd_rssm_scan& d, const Work& w, int which, int t, hipStream_t st);

}  // namespace sdscan

namespace {

using sdscan::Work;

Work work_layout(const sd_rssm_scan& d, float* base) {
  Work w;
  long o = 0;
  const long NT = row_tiles(d);
  const long BU = (long)d.B * d.U;
  auto take = [&](long n) { float* p = base ? base + o : nullptr; o += al64(n); return p; };
  w.x0s = take(d.ks_d * BU);
  w.x1s = take((long)LR_NG * BU);
  w.ops = take(d.ks_d * BU);
  w.ssh = take(NT * MR * (d.D / 8));   // per row tile: 16 rows x D/16 column-tile partials (sized for D/8 tiles)
  w.dotp = take(NT * MR * (d.D / 8));  // the same
  w.dxs = take((long)d.G * d.B * 3 * d.U);
  w.dhin = take((long)d.B * d.D);
  w.gq = take((long)d.B * d.D);
  w.ch = take((long)d.B * d.D);
  w.w1t = take((long)d.SK * d.U);  // _dyn_in1's weight transposed (SK, U): k_logit_rows' gather rows
  w.total = o;
  w.step0 = w.tail = 0;
  w.tailW = nullptr;
  w.tail_ldw = 0;
  return w;
}

constexpr int UH = 256;       // hidden width of the fused path (base.yaml: hidden 256)
constexpr int NU = UH / 128;   // float4 columns per prologue thread over a hidden row

}  // namespace
