// Fused step backward of the imagination (sd_imagine_bwd): the serial walk t = H - 1 .. 0 of the imagined return's
// state gradient (ops.ImagineReturnFn.backward) through prior sample -> img_net -> GRU -> dyn_gru -> dyn_hid ->
// dyn_in0/1/2 -> action sample -> actor, carrying d_stoch[t + 1] / d_deter[t + 1]. Every input is a saved or
// recomputed activation: no sample is drawn again (the noise is redrawn from its Philox counters) and no parameter
// gradient is formed.
//
// 7 launches per step (the per-op walk took 26), all exact-fp32 MFMA contractions (v_mfma_f32_16x16x4_f32,
// gemm16_mainloop) against weight images transposed once per call (k-contiguous B rows):
//   1 k_bw_sample  the prior sample's straight-through backward dl, a team per categorical over the whole chip, then
//     k_bw_prior   16-row tiles: dl . Wl -> [RMSNorm+SiLU backward -> . Wi[l]] -> d_i0; the U-wide intermediates stay
//                  in an LDS panel
//   2 k_bw_i0_gru  d_i0 . Wi0 added into d_deter[t + 1] (now complete), GRU backward in the epilogue: d_gates and
//                  d_deter[t] += dh
//   3 k_bw_gate    d_hh = d_gates . Wg (block diagonal); the epilogue also writes, per 32 columns, the row partials
//                  sum g xhat of dyn_hid's full-row RMSNorm backward
//   4 k_bw_hid     the A loader forms d_hp from d_hh, hp, rh and those partials (summed in order); d_xcat = d_hp . Wsh
//                  and d_deter[t] += d_hp . Wbd as two tile ranges of one grid
//   5 k_bw_act     16-row tiles: the three U-wide RMSNorm+SiLU backwards (d_x0p, d_x1p, d_x2p), d_an = d_x2p . W2, the
//                  action sampler's backward, then back through the actor MLP to d_a0
//   6 k_bw_in      [d_x0p | d_a0] . [W0 ; Wa0[:, SK:]] into d_deter[t] and [d_x1p | d_a0] . [W1 ; Wa0[:, :SK]] into
//                  d_stoch[t]
// Fixed summation order, no atomics: row reductions that cross workgroups go through per-tile partials which the
// consumer sums in order (the forward's `part` scheme), so two calls on the same inputs give the same bits.
#include <climits>

#include "common.h"
#include "dist_core.h"
#include "img_core.h"
#include "philox.h"
#include "sdhip.h"

namespace {
using namespace sdg;

constexpr int UW = 256;       // hidden width (the gate admits U == 256 only)
constexpr int RB = 16;        // rows of a row-kernel tile
constexpr int LDP = UW + 4;   // row stride of the LDS panel
constexpr int HP_PW = 32;     // columns per row partial of dyn_hid's norm backward (one wave's columns in k_bw_gate)
constexpr int XC_KS = 4;      // most K splits of d_xcat = d_hp . Wsh (its slabs in the workspace)

struct BWork {
  float *WlT, *WiT[4], *Wi0T, *WgT, *WshT, *WbdT, *W0T, *W1T, *WaT[4], *Wa0T;  // transposed weight images
  float *dl, *d_i0, *d_gates, *d_hh, *part, *d_xcat, *dcat;                   // one step's intermediates
  float *gn_img, *gn_act;  // the samplers' noise of every step, redrawn once per call: (H, N, SK), (H, N, A)
  long total;
};
long al64b(long n) { return (n + 63) / 64 * 64; }
BWork bwork(const sd_imagine_bwd_desc& d, float* base) {
  BWork w;
  long o = 0;
  auto take = [&](long n) { float* p = base ? base + o : nullptr; o += al64b(n); return p; };
  const long N = d.N, D = d.D, U = d.U, SK = d.SK, Dg = d.D / d.G;
  w.WlT = take(U * SK);
  for (int i = 0; i < 4; ++i) w.WiT[i] = i && i < d.img_layers ? take(U * U) : nullptr;
  w.Wi0T = take(D * U);
  w.WgT = take(D * 3 * Dg);
  w.WshT = take(3 * U * D);
  w.WbdT = take(D * Dg);
  w.W0T = take(D * U);
  w.W1T = take(SK * U);
  for (int i = 0; i < 4; ++i) w.WaT[i] = i && i < d.actor_layers ? take(U * U) : nullptr;
  w.Wa0T = take((SK + D) * U);
  w.dl = take(N * SK);
  w.d_i0 = take(N * U);
  w.d_gates = take(N * 3 * D);
  w.d_hh = take(N * D);
  w.part = take(N * (D / HP_PW));
  w.d_xcat = take(XC_KS * N * 3 * U);  // K-split slabs, summed in order by k_bw_act
  w.dcat = take(N * 3 * U);  // [d_x0p | d_x1p | d_a0]
  w.gn_img = take((long)(d.H1 - 1) * N * SK);
  w.gn_act = take((long)(d.H1 - 1) * N * d.A);
  w.total = o;
  return w;
}

// dst[b][c][r] = src[b][r][c]: src rows of stride lds, dst rows of stride ldd, batch strides sbs / sbd
struct TrJob {
  const float* src;
  float* dst;
  long lds, ldd, sbs, sbd;
  int rows, cols;
};
__global__ __launch_bounds__(256) void k_bw_transpose(TrJob j) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)j.rows * j.cols) return;
  const long r = i / j.cols, c = i % j.cols;
  j.dst[blockIdx.y * j.sbd + c * j.ldd + r] = j.src[blockIdx.y * j.sbs + r * j.lds + c];
}

// K splits of d_xcat = d_hp . Wsh (K = D, whole 32-deep k tiles per split; D % 64 == 0)
__host__ __device__ inline int xc_ks(int D) { return D % (32 * XC_KS) == 0 ? XC_KS : 2; }
SD_DEV void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
SD_DEV uint64_t eff_seed(const sd_imagine_bwd_desc& d) { return d.seed + (d.seed_ptr ? *d.seed_ptr : 0ull); }
// d silu(z) / dz
SD_DEV float dsilu_(float z) {
  const float s = sigmoidf_(z);
  return s * (1.f + z * (1.f - s));
}

// The samplers' noise of steps [t0, t1), redrawn from sd_onehot_sample_bwd's / sd_bnormal_sample_bwd's Philox counters
// in one full-chip launch per call (as sd_imagine_noise does for the forward): the f64 transforms leave the serial
// chain, whose 16-row tiles occupy a quarter of the chip at 1,024 rows.
__global__ __launch_bounds__(256) void k_bw_noise(sd_imagine_bwd_desc d, BWork w, int t0, int t1) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x, per_i = (long)d.N * d.SK, per_a = (long)d.N * d.A;
  const uint64_t seed = eff_seed(d);
  if (i < (t1 - t0) * per_i) {
    const int t = t0 + (int)(i / per_i);
    const long e = i % per_i, m = e / d.SK, k = e % d.SK;
    w.gn_img[t * per_i + e] = sd_gumbel(seed, (uint32_t)d.stream_img, (uint32_t)t, (uint64_t)(m + d.row_offset) * d.SK + k);
  }
  if (i < (t1 - t0) * per_a) {
    const int t = t0 + (int)(i / per_a);
    const long e = i % per_a, m = e / d.A, j = e % d.A;
    const uint64_t idx = (uint64_t)(m + d.row_offset) * d.A + j;
    w.gn_act[t * per_a + e] = d.act_discrete ? sd_gumbel(seed, (uint32_t)d.stream_act, (uint32_t)t, idx)
                                             : sd_normal(seed, (uint32_t)d.stream_act, (uint32_t)t, idx);
  }
}

// ------------------------------------------------------------------------------------------- 16-row panels
// A operand of a row kernel: its LDS panel P[RB][LDP]
struct ALds : AStage<RB> {
  const float* P;
  SD_DEV void load(int k0, int) {
    if (this->live(0)) this->r[0] = ld4(P + this->row(0) * LDP + k0 + 4 * this->kq(0));
  }
};
// P = A . WT^T for a (UW, K) k-contiguous weight image, as two halves of 128 columns (4 waves x 32 columns: 41 KB of
// staging instead of 78); both halves are held in registers until the second main loop has read its A (A may be P).
// A 16-row tile's k step is 16 MFMAs a wave, far less than an L2 round trip, and a row kernel runs one wave per SIMD
// on a quarter of the CUs at 1,024 rows: RG_PF k tiles are kept in flight in registers (gemm16_mainloop_fp), else
// every k step waits out the whole latency (measured: 1.7 us a k tile with one tile in flight).
constexpr int RG_PF = 4;
template <class OpA>
SD_DEV void row_gemm(const OpA& a0, const float* WT, long ldw, int K, float* P) {
  f32x4 acc[2][1][2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    OpA la[RG_PF];
    BRows<128> lb[RG_PF];
#pragma unroll
    for (int u = 0; u < RG_PF; ++u) {
      la[u] = a0;
      lb[u] = BRows<128>(WT, ldw, 128 * h, 128, 0);
    }
    gemm16_mainloop_fp<RB, 128, 16, 32, RG_PF>(la, lb, 0, K, acc[h]);
  }
  const Lane L = lane_ids<128, 32>();
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) P[(4 * L.q + r) * LDP + 128 * h + L.wc * 32 + 16 * j + L.l16] = acc[h][0][j][r];
  __syncthreads();
}
// RMSNorm + SiLU backward of the panel's rows in place (rownorm.hip rms_bwd's arithmetic: dx = r (g - xhat mean(g
// xhat)), g = dz w, dz = dy silu'(xhat w)): thread tid owns row tid / 16, 16 columns; out (row stride ldo, nullable)
// also receives the rows below M
SD_DEV void panel_rms_bwd(float* P, const float* pre, const float* rstd, const float* nw, int M, int m0, float* out,
                          long ldo) {
  const int r = threadIdx.x >> 4, c0 = 16 * (threadIdx.x & 15);
  const bool valid = m0 + r < M;
  const long m = valid ? m0 + r : M - 1;
  const float rs = rstd[m];
  float g[16], xh[16];
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x4 x = ld4(pre + m * UW + c0 + 4 * i), w = ld4(nw + c0 + 4 * i), dy = ld4(P + r * LDP + c0 + 4 * i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xn = x[e] * rs;
      const float dz = dy[e] * dsilu_(xn * w[e]);
      xh[4 * i + e] = xn;
      g[4 * i + e] = dz * w[e];
      dot += g[4 * i + e] * xn;
    }
  }
  dot = group_sum<16>(dot) / (float)UW;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = valid ? rs * (g[4 * i + e] - xh[4 * i + e] * dot) : 0.f;
    st4(P + r * LDP + c0 + 4 * i, y);
    if (out && valid) st4(out + m * ldo + c0 + 4 * i, y);
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------- 1: prior -> d_i0
// 1a: dl = the straight-through sampler's backward of the prior sample, one team of T = Kd lanes per categorical over
// all N S of them. A launch of its own: the team's chain of ~60 dependent cross-lane steps hides only behind many
// waves, and inside the 16-row kernel below (one wave per SIMD, 32 categoricals a thread in turn) it took 75 of that
// kernel's 91 us at 1,024 rows.
template <int T>
__global__ __launch_bounds__(256) void k_bw_sample(sd_imagine_bwd_desc d, BWork w, int t) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x, per = (long)d.N * d.SK;
  if (e >= per) return;  // (whole teams: SK % T == 0 and 256 % T == 0)
  const float dl = st_sample_backward<T>(d.plogit[t * per + e], true, T, d.unimix, w.gn_img[t * per + e],
                                         d.d_stoch[(t + 1) * per + e], (int)(threadIdx.x % T));
  w.dl[e] = dl;
}
// 1b: 16-row tiles: dl . Wl -> [RMSNorm+SiLU backward -> . Wi[l]] -> d_i0
__global__ __launch_bounds__(256) void k_bw_prior(sd_imagine_bwd_desc d, BWork w, int t) {
  __shared__ __attribute__((aligned(16))) float P[RB * LDP];
  const int N = d.N, SK = d.SK, m0 = blockIdx.x * RB;
  {
    APlain<RB> la(w.dl, SK, m0, N, SK);
    row_gemm(la, w.WlT, SK, SK, P);
  }
  for (int i = d.img_layers - 1; i >= 0; --i) {
    panel_rms_bwd(P, d.img_pre[i] + (long)t * N * UW, d.img_rstd[i] + (long)t * N, d.ni[i], N, m0,
                  i ? nullptr : w.d_i0, UW);
    if (i) {
      ALds la;
      la.P = P;
      row_gemm(la, w.WiT[i], UW, UW, P);
    }
  }
}

// ------------------------------------------------------------------------------------------- 64 x 64 tiles
// fn(m, n, acc value) over the tile's elements inside M rows (gemm16_mainloop<64, 64, 32, 32>'s layout: wave (wr, wc)
// holds rows wr 32 + 16 i + 4 q + r, columns wc 32 + 16 j + l16)
template <class F>
SD_DEV void tile_each(const f32x4 (&acc)[2][2], int m0, int n0, int M, F&& fn) {
  const Lane L = lane_ids<64, 32>();
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + L.wr * 32 + 16 * i + 4 * L.q + r, n = n0 + L.wc * 32 + 16 * j + L.l16;
        if (m < M) fn(m, n, acc[i][j][r]);
      }
}

// 2: d_deter[t + 1] += d_i0 . Wi0; GRU backward: d_gates, d_deter[t] += dh. grid (D / 64, N / 64)
__global__ __launch_bounds__(256) void k_bw_i0_gru(sd_imagine_bwd_desc d, BWork w, int t) {
  const int N = d.N, D = d.D, Dg = D / d.G, F = d.SK + D;
  const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64, g = n0 / Dg;
  APlain<64> la(w.d_i0, UW, m0, N, UW);
  BRows<64> lb(w.Wi0T, UW, n0, 64, 0);
  f32x4 acc[2][2];
  gemm16_mainloop<64, 64, 32, 32>(la, lb, 0, UW, acc);
  float* dn = d.d_deter + (long)(t + 1) * N * D;
  float* dc = d.d_deter + (long)t * N * D;
  const float* gates = d.gates + (long)t * N * 3 * D + (long)g * 3 * Dg;
  const float* h = d.feats + (long)t * N * F + d.SK;
  float* dg = w.d_gates + (long)g * 3 * Dg;
  tile_each(acc, m0, n0, N, [&](int m, int n, float v) {
    const long o = (long)m * D + n, b = (long)m * 3 * D + (n - g * Dg);
    const float dv = dn[o] + v;
    dn[o] = dv;
    const GruGrad gg = gru_gate_backward(gates[b], gates[b + Dg], gates[b + 2 * Dg], h[(long)m * F + n], dv);
    dg[b] = gg.dr;
    dg[b + Dg] = gg.dc;
    dg[b + 2 * Dg] = gg.du;
    dc[o] += gg.dh;
  });
}

// 3: d_hh = d_gates . Wg (block g = n0 / Dg); part[(n / 32) N + m] = sum over 32 columns of g xhat. grid (D / 64, N / 64)
__global__ __launch_bounds__(256) void k_bw_gate(sd_imagine_bwd_desc d, BWork w, int t) {
  const int N = d.N, D = d.D, Dg = D / d.G;
  const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64, g = n0 / Dg;
  APlain<64> la(w.d_gates + (long)g * 3 * Dg, 3L * D, m0, N, 3 * Dg);
  BRows<64> lb(w.WgT, 3L * Dg, n0, 64, 0);
  f32x4 acc[2][2];
  gemm16_mainloop<64, 64, 32, 32>(la, lb, 0, 3 * Dg, acc);
  const float* hp = d.hp + (long)t * N * D;
  const float* rh = d.rh + (long)t * N;
  const Lane L = lane_ids<64, 32>();
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + L.wr * 32 + 16 * i + 4 * L.q + r;
      float ss = 0.f;
      if (m < N) {
        const float rs = rh[m];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int n = n0 + L.wc * 32 + 16 * j + L.l16;
          const float v = acc[i][j][r], wv = d.nh[n], xn = hp[(long)m * D + n] * rs;
          w.d_hh[(long)m * D + n] = v;
          ss += v * dsilu_(xn * wv) * wv * xn;
        }
      }
      ss = group_sum<16>(ss);
      if (L.l16 == 0 && m < N) w.part[(long)(n0 / HP_PW + L.wc) * N + m] = ss;
    }
}

// A(m, k) = d_hp[m][c0 + k]: dyn_hid's RMSNorm + SiLU backward of d_hh, the row's mean(g xhat) (dt) and rstd in LDS
struct AHp : AStage<64> {
  const float *dhh, *hp, *nh;
  long D;
  int m0, M, c0;
  float rr[NV], dt[NV];
  f32x4 xr[NV], wv[NV];
  SD_DEV AHp(const float* dhh_, const float* hp_, const float* nh_, long D_, const float* srh, const float* sdot,
             int m0_, int M_, int c0_)
      : dhh(dhh_), hp(hp_), nh(nh_), D(D_), m0(m0_), M(M_), c0(c0_) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      rr[v] = srh[row(v)];
      dt[v] = sdot[row(v)];
    }
  }
  SD_DEV void load(int k0, int) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const long m = m0 + row(v) < M ? m0 + row(v) : M - 1;  // (rows past M: a valid row's values, never stored)
      const int c = c0 + k0 + 4 * kq(v);
      r[v] = ld4(dhh + m * D + c);
      xr[v] = ld4(hp + m * D + c);
      wv[v] = ld4(nh + c);
    }
  }
  SD_DEV void store(float* lds) const {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      f32x4 y;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xn = xr[v][e] * rr[v];
        const float gv = r[v][e] * dsilu_(xn * wv[v][e]) * wv[v][e];
        y[e] = rr[v] * (gv - xn * dt[v]);
      }
      st4(lds + row(v) * LDS_ROW + 4 * kq(v), y);
    }
  }
};

// 4: d_xcat = d_hp . Wsh (the first ks 3U / 64 tiles of the grid: column tile x / ks, K split x % ks of K = D, one
// slab per split: 192 workgroups of 64 k tiles at 1,024 rows would leave a quarter of the CUs idle and one wave per
// SIMD) and d_deter[t] += d_hp . Wbd (the D / 64 tiles after them, K = Dg of the tile's block).
// grid (ks 3U / 64 + D / 64, N / 64)
__global__ __launch_bounds__(256) void k_bw_hid(sd_imagine_bwd_desc d, BWork w, int t) {
  __shared__ float sdot[64], srh[64], red[256];
  const int N = d.N, D = d.D, Dg = D / d.G, np = D / HP_PW, tid = threadIdx.x;
  const int m0 = blockIdx.y * 64, ks = xc_ks(D), nsh = ks * (3 * UW / 64);
  {  // the rows' mean(g xhat) from k_bw_gate's partials: 4 groups of every fourth partial, then the groups in order
    const int row = tid % 64, grp = tid / 64;
    const long m = m0 + row < N ? m0 + row : N - 1;
    float s = 0.f;
#pragma unroll 4
    for (int p = grp; p < np; p += 4) s += w.part[(long)p * N + m];
    red[tid] = s;
    __syncthreads();
    if (tid < 64) {
      sdot[tid] = (((red[tid] + red[64 + tid]) + red[128 + tid]) + red[192 + tid]) / (float)D;
      srh[tid] = d.rh[(long)t * N + m];
    }
    __syncthreads();
  }
  const bool sh = (int)blockIdx.x < nsh;
  const int split = sh ? blockIdx.x % ks : 0;  // d_xcat's K split: columns [split, split + 1) D / ks of d_hp
  const int n0 = (sh ? blockIdx.x / ks : blockIdx.x - nsh) * 64, c0 = sh ? split * (D / ks) : n0 / Dg * Dg;
  const int K = sh ? D / ks : Dg;
  AHp la(w.d_hh, d.hp + (long)t * N * D, d.nh, D, srh, sdot, m0, N, c0);
  BRows<64> lb(sh ? w.WshT + c0 : w.WbdT, sh ? D : Dg, n0, 64, 0);
  f32x4 acc[2][2];
  gemm16_mainloop<64, 64, 32, 32>(la, lb, 0, K, acc);
  if (sh) {
    float* slab = w.d_xcat + (long)split * N * 3 * UW;
    tile_each(acc, m0, n0, N, [&](int m, int n, float v) { slab[(long)m * 3 * UW + n] = v; });
  } else {
    float* dc = d.d_deter + (long)t * N * D;
    tile_each(acc, m0, n0, N, [&](int m, int n, float v) { dc[(long)m * D + n] += v; });
  }
}

// ------------------------------------------------------------------------------------------- 5: d_xcat -> d_a0
template <bool DISC>
__global__ __launch_bounds__(256) void k_bw_act(sd_imagine_bwd_desc d, BWork w, int t) {
  __shared__ __attribute__((aligned(16))) float P[RB * LDP];
  __shared__ float dal[RB][32];
  const int N = d.N, A = d.A, LA = DISC ? A : 2 * A, m0 = blockIdx.x * RB, tid = threadIdx.x;
  const int r = tid >> 4, jj = tid & 15;
  const bool valid = m0 + r < N;
  const long m = valid ? m0 + r : N - 1, tm = (long)t * N + m;
  // the three input branches' norm backwards: d_x0p and d_x1p leave for k_bw_in, d_x2p stays in the panel
  const float* pre[3] = {d.x0p, d.x1p, d.x2p};
  const float* rst[3] = {d.r0, d.r1, d.r2};
  const float* nw[3] = {d.n0, d.n1, d.n2};
#pragma unroll
  for (int b = 0; b < 3; ++b) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
    {
      f32x4 v = ld4(w.d_xcat + m * 3 * UW + b * UW + 16 * jj + 4 * i);
      for (int ks = 1; ks < xc_ks(d.D); ++ks)  // the K-split slabs of k_bw_hid, in order
        v += ld4(w.d_xcat + ((long)ks * N + m) * 3 * UW + b * UW + 16 * jj + 4 * i);
      st4(P + r * LDP + 16 * jj + 4 * i, v);
    }
    __syncthreads();
    panel_rms_bwd(P, pre[b] + (long)t * N * UW, rst[b] + (long)t * N, nw[b], N, m0, b < 2 ? w.dcat + b * UW : nullptr,
                  3 * UW);
  }
  // d_an = d_x2p . W2 (lane jj < A of the row's 16), then the action sampler's backward into dal[r][0 .. LA)
  float dan = 0.f;
  if (jj < A) {
#pragma unroll 8
    for (int u = 0; u < UW; ++u) dan += P[r * LDP + u] * d.W2[u * A + jj];
  }
  const float gna = jj < A ? w.gn_act[tm * A + jj] : 0.f;
  dal[r][jj] = 0.f;
  dal[r][16 + jj] = 0.f;
  __syncthreads();
  if (DISC) {  // the normalisation is the identity on a one-hot
    const bool act = jj < A;
    const float l = act ? d.alogit[tm * A + jj] : 0.f;
    const float dl = st_sample_backward<16>(l, act, A, d.act_unimix, gna, act ? dan : 0.f, jj);
    if (act) dal[r][jj] = dl;
  } else if (jj < A) {
    const BNormal b = bnormal_loc_scale(d.alogit, tm * 2 * A + jj, tm * 2 * A + A + jj);
    float dm, dsd;
    bnormal_sample_backward(b, dan, d.actions[tm * A + jj], gna, d.min_std, d.max_std, dm, dsd);
    dal[r][jj] = dm;
    dal[r][A + jj] = dsd;
  }
  __syncthreads();
  {  // the actor's output layer: d = dal . Wao
    f32x4 y[4] = {};
    for (int o = 0; o < LA; ++o) {
      const float dv = dal[r][o];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x4 wq = ld4(d.Wao + (long)o * UW + 16 * jj + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) y[i][e] += dv * wq[e];
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) st4(P + r * LDP + 16 * jj + 4 * i, y[i]);
  }
  __syncthreads();
  for (int i = d.actor_layers - 1; i >= 0; --i) {
    panel_rms_bwd(P, d.act_pre[i] + (long)t * N * UW, d.act_rstd[i] + (long)t * N, d.na[i], N, m0,
                  i ? nullptr : w.dcat + 2 * UW, 3 * UW);
    if (i) {
      ALds la;
      la.P = P;
      row_gemm(la, w.WaT[i], UW, UW, P);
    }
  }
}

// 6: d_stoch[t] += d_x1p . W1 + d_a0 . Wa0[:, :SK] (column tiles n0 < SK), d_deter[t] += d_x0p . W0 + d_a0 . Wa0[:, SK:].
// grid ((SK + D) / 64, N / 64)
__global__ __launch_bounds__(256) void k_bw_in(sd_imagine_bwd_desc d, BWork w, int t) {
  const int N = d.N, D = d.D, SK = d.SK;
  const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
  const bool st = n0 < SK;
  f32x4 acc[2][2];
  {
    APlain<64> la(w.dcat + (st ? UW : 0), 3 * UW, m0, N, UW);
    BRows<64> lb(st ? w.W1T : w.W0T, UW, st ? n0 : n0 - SK, 64, 0);
    gemm16_mainloop<64, 64, 32, 32>(la, lb, 0, UW, acc);
  }
  {
    APlain<64> la(w.dcat + 2 * UW, 3 * UW, m0, N, UW);
    BRows<64> lb(w.Wa0T, UW, n0, 64, 0);
    gemm16_mainloop<64, 64, 32, 32>(la, lb, 0, UW, acc, true);
  }
  if (st) {
    float* o = d.d_stoch + (long)t * N * SK;
    tile_each(acc, m0, n0, N, [&](int m, int n, float v) { o[(long)m * SK + n] += v; });
  } else {
    float* o = d.d_deter + (long)t * N * D;
    tile_each(acc, m0, n0, N, [&](int m, int n, float v) { o[(long)m * D + n - SK] += v; });
  }
}

// ------------------------------------------------------------------------------------------- host side
// sd_imagine's gate (img.hip ishape) with at least one step to walk
int bshape(const sd_imagine_bwd_desc* d) {
  if (d->N < 1 || d->H1 < 2 || d->U != UW || d->G < 1 || d->D < 1 || d->D % d->G || d->D > 4096) return SD_ESHAPE;
  const int Dg = d->D / d->G;
  if (Dg % 64 || d->SK < 64 || d->SK % 64 || (d->Kd != 16 && d->Kd != 32)) return SD_ESHAPE;
  if (d->A < 1 || (d->act_discrete ? d->A > 16 : 2 * d->A > 32)) return SD_ESHAPE;
  if (d->actor_layers < 1 || d->actor_layers > 4 || d->img_layers < 1 || d->img_layers > 4) return SD_ESHAPE;
  if (bwork(*d, nullptr).total > INT_MAX) return SD_ESHAPE;
  return SD_OK;
}

int transpose(hipStream_t st, const float* src, float* dst, int rows, int cols, long lds, long ldd, int batch = 1,
              long sbs = 0, long sbd = 0) {
  k_bw_transpose<<<dim3(sd_cdiv((long)rows * cols, 256), batch), 256, 0, st>>>(TrJob{src, dst, lds, ldd, sbs, sbd, rows, cols});
  SD_LAUNCH_CHECK();
  return SD_OK;
}

}  // namespace

extern "C" int sd_imagine_bwd_ok(const sd_imagine_bwd_desc* d) { return d && bshape(d) == SD_OK ? 1 : 0; }

extern "C" int sd_imagine_bwd_work_floats(const sd_imagine_bwd_desc* d) {
  if (!d) return SD_EARG;
  const int rc = bshape(d);
  if (rc) return rc;
  return (int)bwork(*d, nullptr).total;
}

extern "C" int sd_imagine_bwd(const sd_imagine_bwd_desc* dp, sd_stream stream_) {
  if (!dp) return SD_EARG;
  const sd_imagine_bwd_desc& d = *dp;
  int rc = bshape(dp);
  if (rc) return rc;  // before any pointer is looked at and before any launch
  const int H = d.H1 - 1, t_end = d.t_end > 0 ? d.t_end : H;
  if (d.t_begin < 0 || d.t_begin >= t_end || t_end > H) return SD_EARG;
  const void* need[] = {d.feats, d.actions, d.x0p, d.x1p, d.x2p, d.r0, d.r1, d.r2, d.hp, d.rh, d.gates, d.plogit,
                        d.alogit, d.d_stoch, d.d_deter, d.work, d.Wao, d.W0, d.n0, d.W1, d.n1, d.W2, d.n2, d.Wh, d.nh,
                        d.Wg, d.Wl};
  for (const void* p : need)
    if (!p) return SD_EARG;
  for (int i = 0; i < d.actor_layers; ++i)
    if (!d.Wa[i] || !d.na[i] || !d.act_pre[i] || !d.act_rstd[i]) return SD_EARG;
  for (int i = 0; i < d.img_layers; ++i)
    if (!d.Wi[i] || !d.ni[i] || !d.img_pre[i] || !d.img_rstd[i]) return SD_EARG;
  for (const void* p : {(const void*)d.feats, (const void*)d.x0p, (const void*)d.x1p, (const void*)d.x2p,
                        (const void*)d.hp, (const void*)d.gates, (const void*)d.d_stoch, (const void*)d.d_deter,
                        (const void*)d.work, (const void*)d.Wao})
    if ((uintptr_t)p & 15) return SD_EALIGN;
  hipStream_t st = (hipStream_t)stream_;
  const BWork w = bwork(d, d.work);
  const int N = d.N, D = d.D, SK = d.SK, G = d.G, Dg = D / G, F = SK + D;
  const long Ig = Dg + 3L * UW;
  // the weight images, once per call
  if ((rc = transpose(st, d.Wl, w.WlT, SK, UW, UW, SK))) return rc;
  for (int i = 1; i < d.img_layers; ++i)
    if ((rc = transpose(st, d.Wi[i], w.WiT[i], UW, UW, UW, UW))) return rc;
  if ((rc = transpose(st, d.Wi[0], w.Wi0T, UW, D, D, UW))) return rc;
  if ((rc = transpose(st, d.Wg, w.WgT, 3 * Dg, Dg, Dg, 3L * Dg, G, 3L * Dg * Dg, 3L * Dg * Dg))) return rc;
  if ((rc = transpose(st, d.Wh + Dg, w.WshT, Dg, 3 * UW, Ig, D, G, Dg * Ig, Dg))) return rc;
  if ((rc = transpose(st, d.Wh, w.WbdT, Dg, Dg, Ig, Dg, G, Dg * Ig, (long)Dg * Dg))) return rc;
  if ((rc = transpose(st, d.W0, w.W0T, UW, D, D, UW))) return rc;
  if ((rc = transpose(st, d.W1, w.W1T, UW, SK, SK, UW))) return rc;
  for (int i = 1; i < d.actor_layers; ++i)
    if ((rc = transpose(st, d.Wa[i], w.WaT[i], UW, UW, UW, UW))) return rc;
  if ((rc = transpose(st, d.Wa[0], w.Wa0T, UW, F, F, UW))) return rc;
  {
    const long n = (long)(t_end - d.t_begin) * N * (SK > d.A ? SK : d.A);
    k_bw_noise<<<sd_cdiv(n, 256), 256, 0, st>>>(d, w, d.t_begin, t_end);
    SD_LAUNCH_CHECK();
  }
  const int rt = sd_cdiv(N, RB), mt = sd_cdiv(N, 64);
  for (int t = t_end - 1; t >= d.t_begin; --t) {
    if (d.Kd == 16)
      k_bw_sample<16><<<sd_cdiv((long)N * SK, 256), 256, 0, st>>>(d, w, t);
    else
      k_bw_sample<32><<<sd_cdiv((long)N * SK, 256), 256, 0, st>>>(d, w, t);
    SD_LAUNCH_CHECK();
    k_bw_prior<<<rt, 256, 0, st>>>(d, w, t);
    SD_LAUNCH_CHECK();
    k_bw_i0_gru<<<dim3(D / 64, mt), 256, 0, st>>>(d, w, t);
    SD_LAUNCH_CHECK();
    k_bw_gate<<<dim3(D / 64, mt), 256, 0, st>>>(d, w, t);
    SD_LAUNCH_CHECK();
    k_bw_hid<<<dim3(xc_ks(D) * (3 * UW / 64) + D / 64, mt), 256, 0, st>>>(d, w, t);
    SD_LAUNCH_CHECK();
    if (d.act_discrete)
      k_bw_act<true><<<rt, 256, 0, st>>>(d, w, t);
    else
      k_bw_act<false><<<rt, 256, 0, st>>>(d, w, t);
    SD_LAUNCH_CHECK();
    k_bw_in<<<dim3(F / 64, mt), 256, 0, st>>>(d, w, t);
    SD_LAUNCH_CHECK();
  }
  return SD_OK;
}
