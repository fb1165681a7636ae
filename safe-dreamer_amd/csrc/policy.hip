// Fused acting step: Dreamer.act after the encoder (dreamer.py:330-357) -> RSSM.obs_step (rssm.py:158-178) ->
// Deter.forward (rssm.py:36-75) -> the actor MLP (networks.py:313-377) and its sample or mode, for B <= 4096 rows as
// 5 + actor_layers launches (sd_policy_step; the per-op path issues ~29 after the encoder):
//   1          k_policy_prelude  everything the step kernels read that does not depend on them, one launch (below)
//   2 3 4 5    the scan's own step kernels at T = 1 (scan.hip, through sdscan::fwd_phase): k_hid, k_gate, k_slab,
//              k_logit_rows. The last step of a scan leaves two operand slots unused, and here they carry the two
//              halves of actor layer 0: k_slab's second problem is deter . Wa0[:, SK:]^T (slabs into x0s, which k_hid
//              has consumed by then), k_logit_rows' "next x1p" gather is sample . Wa0[:, :SK]^T (a one-hot row's
//              product is a gather of rows of the transposed half; slabs into x1s) — no launch of its own re-reads the
//              new state for the actor
//   6 ..       k_policy_layer per actor layer 1 .. L - 1, k_policy_out: row-tiled exact-fp32 MFMA contractions in the
//              scan's style; the prologue sums the slabs (after layer 0) and applies bias, RMSNorm and SiLU; the output
//              kernel's epilogue samples the action or takes its mode.
// No weight-derived image outlives a call: parameters are read in place as f32, and the one transposed image (the
// one-hot half of Wa0) is rebuilt by every prelude. No hazard forces a further launch: each launch reads only what an
// earlier launch (or the caller) wrote, and the buffers reused within a call (x0s, x1s) are rewritten only after their
// one reader has run.
#include "common.h"
#include "dist_core.h"
#include "philox.h"
#include "sdhip.h"

#include "scan_core.h"

namespace {

// one call's intermediates in sd_policy.work: the hoisted inputs, the step kernels' saved activations (the scan writes
// them for its backward; here they are scratch) and the actor's pre-norm rows
struct PWork {
  float *x2, *eproj, *h_in, *x0p, *x1p, *xcat, *r0, *r1, *hp, *hh, *rh, *gates, *op, *oo, *ro, *logit, *pre[2];
  Work scan;  // x0s, x1s, ops, ssh, w1t (the backward's scratch stays null)
  long total;
};

int row_tiles_of(int B) { return (B + MR - 1) / MR; }

PWork pwork(const sd_policy& d, float* base) {
  PWork p;
  long o = 0;
  const long B = d.B, BU = B * UH, BD = B * d.D, nt = row_tiles_of(d.B);
  auto take = [&](long n) { float* q = base ? base + o : nullptr; o += al64(n); return q; };
  p.scan = Work{};
  p.scan.x0s = take(KSM * BU);
  p.scan.x1s = take(LR_NG * BU);
  p.scan.ops = take(KSM * BU);
  p.scan.ssh = take(nt * MR * (d.D / 8));
  p.scan.w1t = take((long)d.SK * UH);  // Wa0[:, :SK]^T: k_logit_rows' gather rows
  p.x2 = take(BU);
  p.eproj = take(BU);
  p.h_in = take(BD);
  p.x0p = take(BU);
  p.x1p = take(BU);
  p.xcat = take(3 * BU);
  p.r0 = take(B);
  p.r1 = take(B);
  p.hp = take(BD);
  p.hh = take(BD);
  p.rh = take(B);
  p.gates = take(3 * BD);
  p.op = take(BU);
  p.oo = take(BU);
  p.ro = take(B);
  p.logit = take(B * d.SK);
  p.pre[0] = take(BU);
  p.pre[1] = take(BU);
  p.total = o;
  return p;
}

int pshape(const sd_policy* d) {
  if (!d) return SD_EARG;
  if (d->B < 1 || d->B > 4096 || d->U != UH || d->G < 1 || d->G > 8 || d->D < 1 || d->D > 4096 || d->D % d->G)
    return SD_ESHAPE;
  const int Dg = d->D / d->G;
  if ((Dg != 256 && Dg != 512) || (d->SK != 512 && d->SK != 1024) || (d->Kd != 16 && d->Kd != 32)) return SD_ESHAPE;
  if (d->A < 1 || (d->act_discrete ? d->A > 16 : 2 * d->A > 32)) return SD_ESHAPE;
  if (d->actor_layers < 1 || d->actor_layers > 4 || d->E < 1 || d->E % 4) return SD_ESHAPE;
  return SD_OK;
}

// ------------------------------------------------------------------------------------------- prelude
// Workgroup roles by blockIdx.x (CT = U / 16 column tiles, nt row tiles of <= 16 rows):
//   [0, CT KSM nt)        slab s of x0p = sel(deter) . W0^T   (k_hid sums the KSM slabs, adds b0, normalises)
//   [.., + CT LR_NG nt)   slab s of x1p = sel(stoch) . W1^T   (LR_NG slabs, as k_logit_rows writes them in a scan)
//   [.., + CT nt)         eproj = embed . Wo[:, D:]^T + bo    (whole K = E in one workgroup: k_logit_rows reads sums)
//   [.., + nt)            x2 = SiLU(RMSNorm(_dyn_in2(action_norm(sel(prev_action)))))  (16 rows each, K = A <= 16: FMAs)
//   [.., + PRE_COPY)      h_in = sel(deter), and w1t = Wa0[:, :SK]^T through 64 x 64 LDS tiles
// sel(): rows whose is_first byte is set read as zero — a select on the A operand, so whatever the caller left in those
// rows (inf, NaN) is never multiplied.
constexpr int PRE_COPY = 64;
constexpr int TP = 64;  // transpose tile
constexpr int pre_lds_floats() { return core_lds_floats<1>() > TP * (TP + 1) ? core_lds_floats<1>() : TP * (TP + 1); }

__global__ __launch_bounds__(NTHR) void k_policy_prelude(sd_policy d, PWork p, int nt) {
  __shared__ __attribute__((aligned(16))) float smem[pre_lds_floats()];
  SD_THREAD_IDS
  const int B = d.B, D = d.D, SK = d.SK, CT = UH / 16, nslab = CT * KSM * nt;
  int i = blockIdx.x;
  if (i < 2 * nslab + CT * nt) {  // ---- the three row-tiled contractions
    const float *A, *W, *bias = nullptr;
    float* out;
    long lda, ldw;
    int K, tile, rtile;
    bool masked = true;
    if (i < 2 * nslab) {
      const bool p1 = i >= nslab;
      if (p1) i -= nslab;
      tile = i % CT;
      const int s = (i / CT) % KSM;
      rtile = i / (CT * KSM);
      const int Kt = p1 ? SK : D;
      K = Kt / KSM;
      A = (p1 ? d.stoch : d.deter) + s * K;
      W = (p1 ? d.W1 : d.W0) + s * K;
      lda = ldw = Kt;
      out = (p1 ? p.scan.x1s : p.scan.x0s) + (long)s * B * UH;
    } else {
      i -= 2 * nslab;
      tile = i % CT;
      rtile = i / CT;
      K = d.E;
      A = d.embed;
      lda = d.E;
      W = d.Wo + D;
      ldw = D + d.E;
      out = p.eproj;
      bias = d.bo;
      masked = false;
    }
    const int rb = rtile * MR, nr = min(MR, B - rb), n0 = tile * 16;
    const int lr = rb + (l16 < nr ? l16 : nr - 1);  // rows past the tile read its last row (results discarded)
    const bool zero = masked && d.is_first[lr] != 0;
    const float* ar = A + (long)lr * lda;
    const float* wr = W + (long)(n0 + l16) * ldw;
    Core<1, 2> core;  // (its accumulator and 8-wave reduction; the k loop below takes any K % 4 == 0)
    core.acc[0] = zero4();
    for (int ch = wave; ch * 16 < K; ch += NW) {
      const int k = ch * 16 + 4 * q;
      f32x4 a = zero4(), b = zero4();
      if (k < K) {
        a = ld4(ar + k);
        b = ld4(wr + k);
      }
      if (zero) a = zero4();
#pragma unroll
      for (int j = 0; j < 4; ++j) core.acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], core.acc[0], 0, 0, 0);
    }
    float* C = smem + NW * 256;
    core.reduce(smem, C, tid, wave, lane);
    if (tid < 256) {
      const int er = tid >> 4, c = tid & 15;
      const float v = C[er * 16 + c];
      if (er < nr) out[(long)(rb + er) * UH + n0 + c] = bias ? v + bias[n0 + c] : v;
    }
    return;
  }
  i -= 2 * nslab + CT * nt;
  if (i < nt) {  // ---- the action branch, 32 threads per row
    const int rb = i * MR, nr = min(MR, B - rb), row = tid >> 5, t32 = tid & 31;
    const bool rv = row < nr;
    const int gr = rb + (rv ? row : nr - 1);
    const bool zero = d.is_first[gr] != 0;
    float an[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float a = (j < d.A && !zero) ? d.prev_action[(long)gr * d.A + j] : 0.f;
      an[j] = a / fmaxf(fabsf(a), 1.f);  // action_norm (rssm.py:44)
    }
    f32x4 x[NU], nv[NU], y[NU];
    ld_row(x, d.b2, t32);
    ld_row(nv, d.n2, t32);
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float* w2 = d.W2 + (long)(4 * t32 + 128 * u + e) * d.A;
        float v = x[u][e];  // b2 first, then j = 0, 1, ...
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (j < d.A) v = fmaf(an[j], w2[j], v);
        x[u][e] = v;
      }
    rms_silu_rows(x, nv, UH, d.eps, rv, y);
    if (rv) st_row(p.x2 + (long)gr * UH, y, UH, t32);
    return;
  }
  i -= nt;  // ---- copies
  const long nD = (long)B * D;
  for (long j = (long)i * NTHR + tid; j < nD; j += (long)PRE_COPY * NTHR)
    p.h_in[j] = d.is_first[j / D] ? 0.f : d.deter[j];
  const float* wa = d.Wa[0];
  const long ldw = (long)SK + D;
  const int tk = SK / TP, ntile = tk * (UH / TP);
  for (int tl = i; tl < ntile; tl += PRE_COPY) {  // w1t[k][c] = Wa0[c][k], k < SK
    const int k0 = (tl % tk) * TP, c0 = (tl / tk) * TP;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TP * TP / 4 / NTHR; ++r) {
      const int e = tid + NTHR * r, c = e / (TP / 4), k4 = (e % (TP / 4)) * 4;
      const f32x4 v = ld4(wa + (long)(c0 + c) * ldw + k0 + k4);
#pragma unroll
      for (int j = 0; j < 4; ++j) smem[(k4 + j) * (TP + 1) + c] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TP * TP / NTHR; ++r) {
      const int e = tid + NTHR * r, k = e / TP, c = e % TP;
      p.scan.w1t[(long)(k0 + k) * UH + c0 + c] = smem[k * (TP + 1) + c];
    }
  }
}

// ------------------------------------------------------------------------------------------- actor tail
// One actor layer's operands. `first`: the layer's input is layer 0's output, still the KSM deter slabs (x0s) and LR_NG
// one-hot slabs (x1s) of the step kernels, summed here in fixed order (deter slabs, one-hot slabs, then bias b_in);
// otherwise pre_in holds the previous layer's pre-norm rows with their bias.
struct ActL {
  const float *pre_in, *b_in, *n_in;  // input rows (B, U) or null; layer 0's bias (first only); the input's norm weight
  const float *W, *b;                 // this layer: (U or NO rows, U), bias
  float* out;                         // pre-norm output rows (B, U) (k_policy_layer)
  int B;
  float eps;
};

// the 16 x U A panel of an actor layer into LDS (row stride U + 4): y = SiLU(RMSNorm(x) n_in), 32 threads per row
template <bool FIRST>
SD_DEV void actor_panel(const ActL& a, const Work& w, int rb, int nr, float* P, int tid) {
  const int row = tid >> 5, t32 = tid & 31;
  const bool rv = row < nr;
  const long gr = rb + (rv ? row : nr - 1);
  f32x4 x[NU], nv[NU], y[NU];
  ld_row(nv, a.n_in, t32);
  if constexpr (FIRST) {
    f32x4 pd[KSM][NU], ps[LR_NG][NU], bv[NU], xs[NU];
    ld_slabs<NU, KSM>(pd, w.x0s + gr * UH, (long)a.B * UH, KSM, t32);
    ld_slabs<NU, LR_NG>(ps, w.x1s + gr * UH, (long)a.B * UH, LR_NG, t32);
    ld_row(bv, a.b_in, t32);
    sum_slabs(x, pd, KSM);
    sum_slabs(xs, ps, LR_NG);
#pragma unroll
    for (int i = 0; i < NU; ++i) x[i] = (x[i] + xs[i]) + bv[i];
  } else {
    ld_row(x, a.pre_in + gr * UH, t32);
  }
  rms_silu_rows(x, nv, UH, a.eps, rv, y);
  st_row(P + row * (UH + 4), y, UH, t32);
}

// pre-norm rows of actor layer i >= 1: out = y . W^T + b. grid (U/16, 1, row tiles)
template <bool FIRST>
__global__ __launch_bounds__(NTHR) void k_policy_layer(ActL a, Work w) {
  extern __shared__ float smem[];
  SD_THREAD_IDS
  const int rb = (int)blockIdx.z * MR, nr = min(MR, a.B - rb), n0 = (int)blockIdx.x * 16;
  Core<1, 2> core;
  const float* wt[1] = {a.W + (long)(n0 + l16) * UH};
  core.load_b(wt, UH / 16, wave, q);
  const float bv = a.b[n0 + (tid & 15)];
  float* P = smem + core_lds_floats<1>();
  actor_panel<FIRST>(a, w, rb, nr, P, tid);
  __syncthreads();
  core.run_lds(P, UH + 4, UH / 16, wave, l16, q);
  float* C = smem + NW * 256;
  core.reduce(smem, C, tid, wave, lane);
  if (tid < 256) {
    const int er = tid >> 4, c = tid & 15;
    if (er < nr) a.out[(long)(rb + er) * UH + n0 + c] = C[er * 16 + c] + bv;
  }
}

// the actor's output layer (NO = 2A or A <= 32 logits: two column tiles, rows past NO repeat row NO - 1 and are
// discarded) and the action: one 32-lane team per row. Sampled (eval = 0): bounded normal tanh(mean) + eps scale
// (distributions.py:217-222) or the unimix one-hot straight-through sample (distributions.py:16-33), noise element
// (row + row_offset) * A + j of stream_act at `step`; eval = 1: tanh(mean), or the one-hot of the first argmax of the
// raw logits (dreamer.py:393-398). grid (1, 1, row tiles)
template <bool FIRST>
__global__ __launch_bounds__(NTHR) void k_policy_out(ActL a, Work w, sd_policy d) {
  extern __shared__ float smem[];
  SD_THREAD_IDS
  const int rb = (int)blockIdx.z * MR, nr = min(MR, a.B - rb);
  const int A = d.A, NO = d.act_discrete ? A : 2 * A;
  Core<2, 2> core;
  const float* wt[2] = {a.W + (long)(l16 < NO ? l16 : NO - 1) * UH, a.W + (long)(16 + l16 < NO ? 16 + l16 : NO - 1) * UH};
  core.load_b(wt, UH / 16, wave, q);
  const int er = tid >> 5, c = tid & 31;
  const long gr = rb + er;
  const bool ok = er < nr, on = c < A;
  const float bv = a.b[c < NO ? c : NO - 1];
  const uint64_t seed = d.seed + (d.seed_ptr ? *d.seed_ptr : 0ull);
  float nz = 0.f;
  if (!d.eval && on) {
    const uint64_t el = (uint64_t)(gr + d.row_offset) * A + c;
    nz = d.act_discrete ? sd_gumbel(seed, (uint32_t)d.stream_act, (uint32_t)d.step, el)
                        : sd_normal(seed, (uint32_t)d.stream_act, (uint32_t)d.step, el);
  }
  float* P = smem + core_lds_floats<2>();
  actor_panel<FIRST>(a, w, rb, nr, P, tid);
  __syncthreads();
  core.run_lds(P, UH + 4, UH / 16, wave, l16, q);
  float* C = smem + NW * 2 * 256;  // 16 x 32
  core.reduce(smem, C, tid, wave, lane);
  const float lo = C[er * 32 + c] + bv;
  if (ok && c < NO && d.actor_logit) d.actor_logit[gr * NO + c] = lo;
  float av;
  if (d.act_discrete) {
    int idx;
    if (d.eval) {
      idx = team_first_max<32>(on ? lo : -INFINITY, on ? c : 0x7fffffff);
      av = c == idx ? 1.f : 0.f;
    } else {
      float pr, pp, nl, ys;
      unimix_forward<32>(lo, on, A, d.act_unimix, pr, pp, nl);
      st_soft<32>(nl, nz, on, ys, idx, c);
      av = ((c == idx ? 1.f : 0.f) - ys) + ys;
    }
  } else {
    const float ls = __shfl(lo, (lane + A) & 63, 64);  // the scale logit of element c (c + A < 32: the same team)
    const float loc = tanhf(lo);
    const float sc = (d.max_std - d.min_std) * sigmoidf_(ls + 2.f) + d.min_std;
    av = d.eval ? loc : loc + nz * sc;
  }
  if (ok && on) d.action[gr * A + c] = av;
}

}  // namespace

extern "C" int sd_policy_step_ok(const sd_policy* d) { return pshape(d) == SD_OK ? 1 : 0; }

extern "C" int sd_policy_step_work_floats(const sd_policy* d) {
  const int rc = pshape(d);
  if (rc) return rc;
  return (int)pwork(*d, nullptr).total;
}

extern "C" int sd_policy_step(const sd_policy* dp, sd_stream stream_) {
  int rc = pshape(dp);
  if (rc) return rc;
  const sd_policy& d = *dp;
  const int L = d.actor_layers;
  const void* need[] = {d.W0, d.b0, d.n0, d.W1, d.b1, d.n1, d.W2, d.b2, d.n2, d.Wh, d.bh, d.nh, d.Wg, d.bg, d.Wo, d.bo,
                        d.no, d.Wl, d.bl, d.Wao, d.bao, d.embed, d.is_first, d.stoch, d.deter, d.prev_action,
                        d.stoch_out, d.deter_out, d.action, d.work};
  for (const void* q : need)
    if (!q) return SD_EARG;
  for (int i = 0; i < L; ++i)
    if (!d.Wa[i] || !d.ba[i] || !d.na[i]) return SD_EARG;
  // read (or written) as float4s
  const void* al16[] = {d.W0, d.b0, d.n0, d.W1, d.b1, d.n1, d.b2, d.n2, d.Wh, d.nh, d.Wg, d.Wo, d.Wl, d.Wao, d.embed,
                        d.stoch, d.deter, d.work, d.Wa[0], d.Wa[1], d.Wa[2], d.Wa[3], d.ba[0], d.na[0], d.na[1],
                        d.na[2], d.na[3]};
  for (const void* q : al16)
    if ((uintptr_t)q & 15) return SD_EARG;
  hipStream_t st = (hipStream_t)stream_;
  const PWork p = pwork(d, d.work);
  const int nt = row_tiles_of(d.B), CT = UH / 16;
  k_policy_prelude<<<2 * CT * KSM * nt + CT * nt + nt + PRE_COPY, NTHR, 0, st>>>(d, p, nt);
  SD_LAUNCH_CHECK();
  // the step kernels at T = 1 on the reset-selected state; the saved activations a scan keeps are scratch here
  sd_rssm_scan s{};
  s.B = d.B, s.T = 1, s.D = d.D, s.U = d.U, s.SK = d.SK, s.Kd = d.Kd, s.G = d.G, s.ks_d = KSM;
  s.eps = d.eps, s.unimix = d.unimix, s.seed = d.seed, s.seed_ptr = d.seed_ptr, s.stream_id = d.stream_post;
  s.group_offset = d.row_offset * (d.SK / d.Kd);
  s.W0 = d.W0, s.b0 = d.b0, s.n0 = d.n0, s.W1 = d.W1, s.b1 = d.b1, s.n1 = d.n1;
  s.Wh = d.Wh, s.bh = d.bh, s.nh = d.nh, s.Wg = d.Wg, s.bg = d.bg;
  s.WoD = d.Wo, s.ld_wod = (long)d.D + d.E, s.no = d.no, s.Wl = d.Wl, s.bl = d.bl;
  s.reset = d.is_first, s.x2 = p.x2, s.eproj = p.eproj;
  s.h_in = p.h_in, s.x0p = p.x0p, s.x1p = p.x1p, s.r0 = p.r0, s.r1 = p.r1, s.xcat = p.xcat, s.hp = p.hp, s.hh = p.hh;
  s.rh = p.rh, s.gates = p.gates, s.deter = d.deter_out, s.op = p.op, s.oo = p.oo, s.ro = p.ro;
  s.logit = d.logit ? d.logit : p.logit, s.stoch = d.stoch_out;
  s.work = d.work;
  Work w = p.scan;
  w.step0 = d.step, w.tail = 1, w.tailW = d.Wa[0] + d.SK, w.tail_ldw = (long)d.SK + d.D;
  for (int which = 1; which < 5; ++which) {
    rc = sdscan::fwd_phase(s, w, which, 0, st);
    if (rc) return rc;
  }
  // actor layers 1 .. L - 1, then the output layer and the action
  const size_t lds_layer = (core_lds_floats<1>() + MR * (UH + 4)) * 4, lds_out = (core_lds_floats<2>() + MR * (UH + 4)) * 4;
  for (int i = 1; i <= L; ++i) {
    const bool first = i == 1, last = i == L;
    const ActL a{first ? nullptr : p.pre[(i - 1) & 1], d.ba[0], d.na[i - 1], last ? d.Wao : d.Wa[i],
                 last ? d.bao : d.ba[i], p.pre[i & 1], d.B, d.eps};
    if (last) {
      if (first) k_policy_out<true><<<dim3(1, 1, nt), NTHR, lds_out, st>>>(a, w, d);
      else k_policy_out<false><<<dim3(1, 1, nt), NTHR, lds_out, st>>>(a, w, d);
    } else {
      if (first) k_policy_layer<true><<<dim3(CT, 1, nt), NTHR, lds_layer, st>>>(a, w);
      else k_policy_layer<false><<<dim3(CT, 1, nt), NTHR, lds_layer, st>>>(a, w);
    }
    SD_LAUNCH_CHECK();
  }
  return SD_OK;
}
