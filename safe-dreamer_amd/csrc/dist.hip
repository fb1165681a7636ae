// Distribution heads, latent sampling, KL and the GRU-style gate of the RSSM.
//
//  * one-hot straight-through sampler with unimix (OneHotDist.__init__/rsample, distributions.py:16-33 +
//    torch F.gumbel_softmax(hard=True)): one team of K lanes per categorical, noise generated in-kernel (philox.h);
//    backward recomputes everything from the logits (no saved soft samples);
//  * categorical KL on raw logits, summed over the S latents and clipped at free nats (rssm.py:222-230,
//    distributions.py:266-271); unimix entropy for the dyn/rep entropy metrics (dreamer.py:575-576);
//  * symexp two-hot: mode (distributions.py:78-98) and log_prob (100-129) fwd/bwd, one wave per 255-bin row;
//  * bounded normal (distributions.py:217-222): sample, log_prob, entropy fwd/bwd; discrete-actor log_prob/entropy;
//  * Bernoulli continue head (torchd.Bernoulli(logits)): log_prob fwd/bwd;
//  * Deter gates (rssm.py:65-75): r = sigmoid, c = tanh(r*c), u = sigmoid(u-1), h' = u*c + (1-u)*h, fwd/bwd.
//
// Each family states its device math once and its kernels are that math plus their loads and stores: OneHot (a team's
// unimix categorical) for the one-hot heads, WaveRow / row_softmax64 / TwoHot / twohot_mode / ValuePair for the two-hot
// ones, bnormal_loc_scale for the bounded normal. The two KL kernels each spell out their double softmax: any shared
// function that also gives the backward's pb makes hipcc lay out kl_fwd's loop otherwise (2 VGPRs and 2 SGPRs fewer,
// three instructions fewer), and one that does not is of no use to the backward. The host side is launch, with_team and
// the two-hot shape predicate; every entry point is its early return, its guard and one launch.
#include <type_traits>

#include "common.h"
#include "philox.h"
#include "sdhip.h"
#include "dist_core.h"

namespace {

// ---------------------------------------------------------------- one-hot heads (one team of T lanes per categorical)
// Lane lt of team g holds logit lt of categorical g (lanes >= K idle): p = softmax(l), pp its unimix, nl the normalised
// unimix logits. The teams with g past the last categorical exit before load(); whole teams exit together.
template <int T>
struct OneHot {
  const int lt = threadIdx.x % T;
  const long g = ((long)blockIdx.x * blockDim.x + threadIdx.x) / T;
  bool act;         // act, p, pp, nl: set by load(), which every kernel calls right after its exit test
  float p, pp, nl;
  SD_DEV void load(const float* logits, int K, float unimix) {
    act = lt < K;
    const float l = act ? logits[g * K + lt] : 0.f;
    unimix_forward<T>(l, act, K, unimix, p, pp, nl);
  }
  // the straight-through sample's soft values and index, the Gumbel noise drawn from the categorical's Philox counters
  SD_DEV void sample(int K, uint64_t seed, uint32_t stream, uint32_t step, long group_offset, float& ys,
                     int& idx) const {
    const float gn = act ? sd_gumbel(seed, stream, step, (uint64_t)(g + group_offset) * K + lt) : 0.f;
    st_soft<T>(nl, gn, act, ys, idx, lt);
  }
  // argmax of the action one-hot (value.max(-1)[1]: first max)
  SD_DEV int chosen(const float* action, int K) const {
    return team_first_max<T>(act ? action[g * K + lt] : -INFINITY, act ? lt : 0x7fffffff);
  }
  SD_DEV float backward(float dnl, float unimix) const { return unimix_backward<T>(dnl, p, pp, nl, act, unimix); }
};

template <int T>
__global__ void onehot_sample_fwd(const float* __restrict__ logits, float* __restrict__ out, int* __restrict__ index,
                                  float* __restrict__ entropy, long groups, int K, float unimix, uint64_t seed,
                                  uint32_t stream, uint32_t step, long group_offset, const uint64_t* seed_ptr) {
  if (seed_ptr) seed += *seed_ptr;
  OneHot<T> c;
  if (c.g >= groups) return;
  c.load(logits, K, unimix);
  if (entropy) {
    const float h = group_sum<T>(c.act ? -expf(c.nl) * c.nl : 0.f);
    if (c.lt == 0) entropy[c.g] = h;
  }
  if (!out) return;
  float ys;
  int idx;
  c.sample(K, seed, stream, step, group_offset, ys, idx);
  if (c.act) {
    const float hard = c.lt == idx ? 1.f : 0.f;
    out[c.g * K + c.lt] = (hard - ys) + ys;
  }
  if (index && c.lt == 0) index[c.g] = idx;
}

template <int T>
__global__ void onehot_sample_bwd(const float* __restrict__ logits, const float* __restrict__ dout,
                                  float* __restrict__ dlogits, long groups, int K, float unimix, uint64_t seed,
                                  uint32_t stream, uint32_t step, long group_offset, int accumulate,
                                  const uint64_t* seed_ptr) {
  if (seed_ptr) seed += *seed_ptr;
  OneHot<T> c;
  if (c.g >= groups) return;
  c.act = c.lt < K;
  const float l = c.act ? logits[c.g * K + c.lt] : 0.f;
  const float gn = c.act ? sd_gumbel(seed, stream, step, (uint64_t)(c.g + group_offset) * K + c.lt) : 0.f;
  const float d = c.act ? dout[c.g * K + c.lt] : 0.f;
  const float dl = st_sample_backward<T>(l, c.act, K, unimix, gn, d, c.lt);
  if (c.act) dlogits[c.g * K + c.lt] = accumulate ? dlogits[c.g * K + c.lt] + dl : dl;
}

// discrete actor: logp(a) = nl[argmax a], entropy = -sum exp(nl) nl  (OneHotCategorical.log_prob / entropy)
template <int T>
__global__ void onehot_logp_ent_fwd(const float* __restrict__ logits, const float* __restrict__ action,
                                    float* __restrict__ logp, float* __restrict__ ent, long rows, int K, float unimix) {
  OneHot<T> c;
  if (c.g >= rows) return;
  c.load(logits, K, unimix);
  const int bi = c.chosen(action, K);
  const float sel = group_sum<T>(c.lt == bi ? c.nl : 0.f);
  const float h = group_sum<T>(c.act ? -expf(c.nl) * c.nl : 0.f);
  if (c.lt == 0) { logp[c.g] = sel; ent[c.g] = h; }
}

template <int T>
__global__ void onehot_logp_ent_bwd(const float* __restrict__ logits, const float* __restrict__ action,
                                    const float* __restrict__ glogp, const float* __restrict__ gent,
                                    float* __restrict__ dlogits, long rows, int K, float unimix) {
  OneHot<T> c;
  if (c.g >= rows) return;
  c.load(logits, K, unimix);
  const int bi = c.chosen(action, K);
  const float s = c.act ? expf(c.nl) : 0.f;
  const float h = group_sum<T>(c.act ? -s * c.nl : 0.f);
  const float gl = glogp ? glogp[c.g] : 0.f, ge = gent ? gent[c.g] : 0.f;
  // d logp / d nl = onehot(bi);  d H / d nl_k = -s_k (1 + nl_k + H)   (probs = softmax(nl))
  const float dnl = c.act ? (c.lt == bi ? gl : 0.f) + ge * (-s * (1.f + c.nl + h)) : 0.f;
  const float dl = c.backward(dnl, unimix);
  if (c.act) dlogits[c.g * K + c.lt] = dl;
}

// ---------------------------------------------------------------- KL (raw logits) summed over S, per row
template <int T>
__global__ void kl_fwd(const float* __restrict__ post, const float* __restrict__ prior, float* __restrict__ kl_row,
                       float* __restrict__ dyn, float* __restrict__ rep, float free_nats, int rows, int S, int K) {
  __shared__ float red[4];
  const int teams = 256 / T;
  const int team = threadIdx.x / T, lt = threadIdx.x % T;
  const bool act = lt < K;
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    float acc = 0.f;
    for (int s = team; s < S; s += teams) {
      const long o = ((long)r * S + s) * K + lt;
      const float a = act ? post[o] : -INFINITY, b = act ? prior[o] : -INFINITY;
      const float ma = group_max<T>(a), mb = group_max<T>(b);
      const float ea = act ? expf(a - ma) : 0.f, eb = act ? expf(b - mb) : 0.f;
      const float sa = group_sum<T>(ea), sb = group_sum<T>(eb);
      const float lpa = a - ma - logf(sa), lpb = b - mb - logf(sb);
      const float pa = ea / sa;
      const float kg = group_sum<T>(act ? pa * (lpa - lpb) : 0.f);
      if (lt == 0) acc += kg;
    }
    const float tot = block_sum<256>(acc, red);
    if (threadIdx.x == 0) {
      kl_row[r] = tot;
      const float cl = tot < free_nats ? free_nats : tot;  // torch.clamp(min=free): NaN stays NaN
      if (dyn) dyn[r] = cl;
      if (rep) rep[r] = cl;
    }
    __syncthreads();
  }
}

// d rep / d post = g_rep[r] * 1[kl_r >= free] * pa (lpa - lpb - kl_s) ;  d dyn / d prior = g_dyn[r] * 1[..] * (pb - pa)
template <int T>
__global__ void kl_bwd(const float* __restrict__ post, const float* __restrict__ prior, const float* __restrict__ kl_row,
                       const float* __restrict__ g_rep, const float* __restrict__ g_dyn, float free_nats,
                       float* __restrict__ d_post, float* __restrict__ d_prior, int rows, int S, int K, int acc_post,
                       int acc_prior) {
  const long g = ((long)blockIdx.x * blockDim.x + threadIdx.x) / T;
  const int lt = threadIdx.x % T;
  if (g >= (long)rows * S) return;
  const int r = (int)(g / S);
  const bool act = lt < K;
  const long o = g * K + lt;
  const float a = act ? post[o] : -INFINITY, b = act ? prior[o] : -INFINITY;
  const float ma = group_max<T>(a), mb = group_max<T>(b);
  const float ea = act ? expf(a - ma) : 0.f, eb = act ? expf(b - mb) : 0.f;
  const float sa = group_sum<T>(ea), sb = group_sum<T>(eb);
  const float lpa = a - ma - logf(sa), lpb = b - mb - logf(sb);
  const float pa = ea / sa, pb = eb / sb;
  const float kg = group_sum<T>(act ? pa * (lpa - lpb) : 0.f);
  const bool pass = kl_row[r] >= free_nats;  // torch.clip(min=free) passes the gradient where x >= min
  if (!act) return;
  if (d_post) {
    const float v = pass && g_rep ? g_rep[r] * pa * (lpa - lpb - kg) : 0.f;
    d_post[o] = acc_post ? d_post[o] + v : v;
  }
  if (d_prior) {
    const float v = pass && g_dyn ? g_dyn[r] * (pb - pa) : 0.f;
    d_prior[o] = acc_prior ? d_prior[o] + v : v;
  }
}

// ---------------------------------------------------------------- symexp two-hot (one wave per row)
// wave `wave` of a 256-thread block works on row r = 4 * block + wave; the waves with r >= rows exit at once
struct WaveRow {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + wave;
};

SD_DEV void row_softmax64(const float* l, int NB, float (&p)[4], float& lse, int lane) {
  float v[4];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = lane + 64 * j;
    v[j] = c < NB ? l[c] : -INFINITY;
    m = fmaxf(m, v[j]);
  }
  m = wave_max(m);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = lane + 64 * j;
    p[j] = c < NB ? expf(v[j] - m) : 0.f;
    s += p[j];
  }
  s = wave_sum(s);
#pragma unroll
  for (int j = 0; j < 4; ++j) p[j] /= s;
  lse = m + logf(s);
}

// mode = p[c] b[c] + sum_i (p[c-1-i] b[c-1-i] + p[c+1+i] b[c+1+i]),  c = (NB-1)/2  (NB odd): twohot_mode stages the
// row's p in sp (the wave's 256 floats of LDS) and sums the +- pairs on every lane; value() adds the centre bin. The
// forward (lane 0) and the backward (every lane) both take the mode from here, so they hold the same value.
struct TwoHotMode {
  int c;
  float acc;
  SD_DEV float value(const float* sp, const float* bins) const { return sp[c] * bins[c] + acc; }
};
SD_DEV TwoHotMode twohot_mode(float* sp, const float (&p)[4], const float* bins, int NB, int lane) {
#pragma unroll
  for (int j = 0; j < 4; ++j) sp[lane + 64 * j] = p[j];
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  const int c = (NB - 1) / 2;
  float acc = 0.f;
  for (int i = lane; i < c; i += 64) {
    const float lo = sp[c - 1 - i] * bins[c - 1 - i];
    const float hi = sp[c + 1 + i] * bins[c + 1 + i];
    acc += lo + hi;
  }
  return {c, wave_sum(acc)};
}

__global__ void twohot_mode_kernel(const float* __restrict__ logits, const float* __restrict__ bins,
                                   float* __restrict__ out, long rows, int NB) {
  __shared__ float sp[4][256];
  const WaveRow w;
  if (w.r >= rows) return;
  float p[4], lse;
  row_softmax64(logits + w.r * NB, NB, p, lse, w.lane);
  const TwoHotMode m = twohot_mode(sp[w.wave], p, bins, NB, w.lane);
  if (w.lane == 0) out[w.r] = m.value(sp[w.wave], bins);
}

// d mode / d logits[j] = p[j] (bins[j] - mode), times the row's upstream gradient
__global__ void twohot_mode_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ bins,
                                       const float* __restrict__ dout, float* __restrict__ dlogits, long rows, int NB) {
  __shared__ float sp[4][256];
  const WaveRow w;
  if (w.r >= rows) return;
  float p[4], lse;
  row_softmax64(logits + w.r * NB, NB, p, lse, w.lane);
  const float mode = twohot_mode(sp[w.wave], p, bins, NB, w.lane).value(sp[w.wave], bins);
  const float d = dout[w.r];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = w.lane + 64 * j;
    if (col < NB) dlogits[w.r * NB + col] = p[j] * (bins[col] - mode) * d;
  }
}

// The two-hot encoding of a target: weight wb on bin `below`, wa on bin `above`.
struct TwoHot {
  int below, above;
  float wb, wa;
  // log_prob of the target under logits l with log-sum-exp lse
  SD_DEV float logp(const float* l, float lse) const {
    float v = wb * (l[below] - lse);
    v += wa * (l[above] - lse);
    return v;
  }
  // d logp / d l[c], p = softmax(l)[c]
  SD_DEV float grad(int c, float p) const {
    const float td = (c == below ? wb : 0.f) + (c == above ? wa : 0.f);
    return td - p * (wb + wa);
  }
};

SD_DEV TwoHot twohot_target(const float* bins, int NB, float t, int lane) {
  // below = #(bins <= t) - 1, above = NB - #(bins > t), clamped (distributions.py:106-109)
  int cle = 0, cgt = 0;
  for (int c = lane; c < NB; c += 64) {
    const float b = bins[c];
    cle += b <= t ? 1 : 0;
    cgt += b > t ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cle += __shfl_xor(cle, o, 64);
    cgt += __shfl_xor(cgt, o, 64);
  }
  TwoHot h;
  h.below = min(max(cle - 1, 0), NB - 1);
  h.above = min(max(NB - cgt, 0), NB - 1);
  const bool eq = h.below == h.above;
  const float db = eq ? 1.f : fabsf(bins[h.below] - t);
  const float da = eq ? 1.f : fabsf(bins[h.above] - t);
  const float tot = db + da;
  h.wb = da / tot;
  h.wa = db / tot;
  return h;
}

__global__ void twohot_logp_fwd(const float* __restrict__ logits, const float* __restrict__ bins,
                                const float* __restrict__ target, float* __restrict__ logp, long rows, int NB) {
  const WaveRow w;
  if (w.r >= rows) return;
  const float* l = logits + w.r * NB;
  float p[4], lse;
  row_softmax64(l, NB, p, lse, w.lane);
  const TwoHot h = twohot_target(bins, NB, target[w.r], w.lane);
  if (w.lane == 0) logp[w.r] = h.logp(l, lse);
}

__global__ void twohot_logp_bwd(const float* __restrict__ logits, const float* __restrict__ bins,
                                const float* __restrict__ target, const float* __restrict__ glogp,
                                float* __restrict__ dlogits, long rows, int NB, int accumulate) {
  const WaveRow w;
  if (w.r >= rows) return;
  float p[4], lse;
  row_softmax64(logits + w.r * NB, NB, p, lse, w.lane);
  const TwoHot h = twohot_target(bins, NB, target[w.r], w.lane);
  const float gsc = glogp[w.r];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = w.lane + 64 * j;
    if (c < NB) {
      const float v = gsc * h.grad(c, p[j]);
      float* d = dlogits + w.r * NB + c;
      *d = accumulate ? *d + v : v;
    }
  }
}

// The value-loss term of one row: two targets (the return and the slow critic's value) under one softmax of the value
// head's logits l. Forward -logp(ret) - logp(slow), in two steps so that a kernel reads the four logits first and
// negates where it weights the term (the order its loads and arithmetic always had); backward, for the row's
// d loss / d term g, the sum of the two log-prob gradients in one pass:
// g (td_ret - p tsum_ret) + g (td_slow - p tsum_slow).
struct ValuePair {
  TwoHot ret, slow;
  struct LogP {
    float lr, ls;
    SD_DEV float loss() const { return -lr - ls; }
  };
  SD_DEV LogP logp(const float* l, float lse) const {
    const float lr = ret.logp(l, lse);
    const float ls = slow.logp(l, lse);
    return {lr, ls};
  }
  SD_DEV float grad(float g, int c, float p) const { return g * ret.grad(c, p) + g * slow.grad(c, p); }
};

// Replay-value loss (dreamer.py:652-658): row r's term w[r] * (-logp(ret[r]) - logp(slow[r])) under the TwoHot head
// logits (distributions.py:100-129), and its logits gradient for a given d loss / d term (one wave per row), with
// g = -w[r] * gscale[0] * inv_n (gscale: device scalar, d total / d mean).
// replay-value rows (dreamer.py:638-658): loss row r = (b, t < Tr) reads logits / slow / last row b * Tl + t (the value
// head ran on all Tl posterior steps; Tr = Tl - 1 of them have a return) and ret[r]; weight = 1 - last.
__global__ void repval_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ bins,
                                  const float* __restrict__ ret, const float* __restrict__ slow,
                                  const float* __restrict__ last, float* __restrict__ row_loss, long rows, int Tl,
                                  int Tr, int NB) {
  const WaveRow w;
  if (w.r >= rows) return;
  const long lr_ = (w.r / Tr) * Tl + w.r % Tr;
  const float* l = logits + lr_ * NB;
  float p[4], lse;
  row_softmax64(l, NB, p, lse, w.lane);
  const ValuePair v{twohot_target(bins, NB, ret[w.r], w.lane), twohot_target(bins, NB, slow[lr_], w.lane)};
  if (w.lane == 0) {
    const ValuePair::LogP lp = v.logp(l, lse);
    row_loss[w.r] = (1.f - last[lr_]) * lp.loss();
  }
}

// d logits of the mean of the rows above, for all B * Tl logits rows (zero on the rows without a return)
__global__ void repval_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ bins,
                                  const float* __restrict__ ret, const float* __restrict__ slow,
                                  const float* __restrict__ last, const float* __restrict__ gscale, float inv_n,
                                  float* __restrict__ dlogits, long lrows, int Tl, int Tr, int NB) {
  const WaveRow w;
  const long lr_ = w.r;
  if (lr_ >= lrows) return;
  const int t = (int)(lr_ % Tl);
  if (t >= Tr) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (w.lane + 64 * j < NB) dlogits[lr_ * NB + w.lane + 64 * j] = 0.f;
    return;
  }
  const long r = (lr_ / Tl) * Tr + t;
  float p[4], lse;
  row_softmax64(logits + lr_ * NB, NB, p, lse, w.lane);
  const ValuePair v{twohot_target(bins, NB, ret[r], w.lane), twohot_target(bins, NB, slow[lr_], w.lane)};
  const float g = -(1.f - last[lr_]) * (gscale[0] * inv_n);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = w.lane + 64 * j;
    if (c < NB) dlogits[lr_ * NB + c] = v.grad(g, c, p[j]);
  }
}

// imagined actor-critic losses (dreamer.py:623-636, 653-671) on H * N time-major rows r = t * N + n, the returns /
// weights batch-major (n, t), the values time-major (t, n): adv = (ret[n, t] - val[t, n]) / scale[0] (metrics),
// value row  = w[n, t] * (-logp(vl[r], ret[n, t]) - logp(vl[r], slow[r]))   (TwoHot, distributions.py:100-129),
// policy row = w[n, t] * -(logpi[r] * adv + coef * ent[r]).  One wave per row.
__global__ void imag_ac_fwd_kernel(const float* __restrict__ vl, const float* __restrict__ bins,
                                   const float* __restrict__ ret, const float* __restrict__ slow,
                                   const float* __restrict__ w, const float* __restrict__ val,
                                   const float* __restrict__ scale, const float* __restrict__ logpi,
                                   const float* __restrict__ ent, float coef, long N, int H, int H1, int NB,
                                   float* __restrict__ rows_v, float* __restrict__ rows_p, float* __restrict__ adv) {
  const WaveRow wr;
  const long r = wr.r;
  if (r >= N * H) return;
  const long n = r % N;
  const int t = (int)(r / N);
  const float* l = vl + r * NB;
  const float rt = ret[n * H + t];
  float p[4], lse;
  row_softmax64(l, NB, p, lse, wr.lane);
  const ValuePair v{twohot_target(bins, NB, rt, wr.lane), twohot_target(bins, NB, slow[r], wr.lane)};
  if (wr.lane == 0) {
    const ValuePair::LogP lp = v.logp(l, lse);
    const float wt = w[n * H1 + t];
    const float a = (rt - val[(long)t * N + n]) / scale[0];
    rows_v[r] = wt * lp.loss();
    rows_p[r] = wt * -(logpi[r] * a + coef * ent[r]);
    adv[n * H + t] = a;
  }
}
// d vl (value loss, both log-prob terms), d logpi and d ent (policy loss); g = (policy, value) upstream gradients
__global__ void imag_ac_bwd_kernel(const float* __restrict__ vl, const float* __restrict__ bins,
                                   const float* __restrict__ ret, const float* __restrict__ slow,
                                   const float* __restrict__ w, const float* __restrict__ adv,
                                   const float* __restrict__ gp, const float* __restrict__ gv, float sp, float sv,
                                   float coef, float inv_n, long N, int H, int H1, int NB, float* __restrict__ dvl,
                                   float* __restrict__ dlogpi, float* __restrict__ dent) {
  const WaveRow wr;
  const long r = wr.r;
  if (r >= N * H) return;
  const long n = r % N;
  const int t = (int)(r / N);
  float p[4], lse;
  row_softmax64(vl + r * NB, NB, p, lse, wr.lane);
  const ValuePair v{twohot_target(bins, NB, ret[n * H + t], wr.lane), twohot_target(bins, NB, slow[r], wr.lane)};
  const float wt = w[n * H1 + t];
  const float g = -wt * ((gv ? gv[0] * sv : 0.f) * inv_n);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = wr.lane + 64 * j;
    if (c < NB) dvl[r * NB + c] = v.grad(g, c, p[j]);
  }
  if (wr.lane == 0) {
    const float gg = -wt * ((gp ? gp[0] * sp : 0.f) * inv_n);
    dlogpi[r] = gg * adv[n * H + t];
    dent[r] = gg * coef;
  }
}

// ---------------------------------------------------------------- bounded normal actor
// (BNormal, bnormal_loc_scale, bnormal_sample_backward: dist_core.h)
__global__ void bnormal_sample(const float* __restrict__ x, float* __restrict__ action, long rows, int A, float min_std,
                               float max_std, uint64_t seed, uint32_t stream, uint32_t step, long row_offset,
                               const uint64_t* seed_ptr) {
  if (seed_ptr) seed += *seed_ptr;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * A) return;
  const long r = t / A;
  const int j = (int)(t % A);
  const BNormal b = bnormal_loc_scale(x, r * 2 * A + j, r * 2 * A + A + j);
  const float sc = b.scale(min_std, max_std);
  const float eps = sd_normal(seed, stream, step, (uint64_t)(r + row_offset) * A + j);
  action[t] = b.loc + eps * sc;
}

// Reparameterised gradient of the sampled, normalised action a / max(|a|, 1) (the divisor a constant, rssm.py:44):
// a = loc + eps sc, so d loc = d a and d sc = d a eps, eps drawn again from bnormal_sample's Philox counters.
__global__ void bnormal_sample_bwd(const float* __restrict__ d_an, const float* __restrict__ x,
                                   const float* __restrict__ action, float* __restrict__ dx, long rows, int A,
                                   float min_std, float max_std, uint64_t seed, uint32_t stream, uint32_t step,
                                   long row_offset, const uint64_t* seed_ptr) {
  if (seed_ptr) seed += *seed_ptr;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * A) return;
  const long r = t / A;
  const int j = (int)(t % A);
  const BNormal b = bnormal_loc_scale(x, r * 2 * A + j, r * 2 * A + A + j);
  const float eps = sd_normal(seed, stream, step, (uint64_t)(r + row_offset) * A + j);
  bnormal_sample_backward(b, d_an[t], action[t], eps, min_std, max_std, dx[r * 2 * A + j], dx[r * 2 * A + A + j]);
}

__global__ void bnormal_logp_ent_fwd(const float* __restrict__ x, const float* __restrict__ action,
                                     float* __restrict__ logp, float* __restrict__ ent, long rows, int A, float min_std,
                                     float max_std) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const float c0 = 0.91893853320467274178f;  // log(sqrt(2*pi))
  float lp = 0.f, h = 0.f;
  for (int j = 0; j < A; ++j) {
    const BNormal b = bnormal_loc_scale(x, r * 2 * A + j, r * 2 * A + A + j);
    const float sc = b.scale(min_std, max_std);
    const float d = action[r * A + j] - b.loc;
    lp += -(d * d) / (2.f * sc * sc) - logf(sc) - c0;
    h += 0.5f + c0 + logf(sc);
  }
  logp[r] = lp;
  ent[r] = h;
}

__global__ void bnormal_logp_ent_bwd(const float* __restrict__ x, const float* __restrict__ action,
                                     const float* __restrict__ glogp, const float* __restrict__ gent,
                                     float* __restrict__ dx, long rows, int A, float min_std, float max_std) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * A) return;
  const long r = t / A;
  const int j = (int)(t % A);
  const BNormal b = bnormal_loc_scale(x, r * 2 * A + j, r * 2 * A + A + j);
  const float sc = b.scale(min_std, max_std);
  const float d = action[r * A + j] - b.loc;
  const float gl = glogp ? glogp[r] : 0.f, ge = gent ? gent[r] : 0.f;
  const float d_loc = gl * d / (sc * sc);
  const float d_sc = gl * (d * d / (sc * sc * sc) - 1.f / sc) + ge / sc;
  dx[r * 2 * A + j] = d_loc * (1.f - b.loc * b.loc);
  dx[r * 2 * A + A + j] = d_sc * (max_std - min_std) * b.sg * (1.f - b.sg);
}

// ---------------------------------------------------------------- Bernoulli(logits) continue head, 1 logit/row
__global__ void bernoulli_fwd(const float* __restrict__ logit, const float* __restrict__ value, float* __restrict__ logp,
                              float* __restrict__ mean, long rows) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const float x = logit[r];
  if (mean) mean[r] = sigmoidf_(x);
  if (logp) {
    const float y = value[r];
    const float mx = fmaxf(-x, 0.f);  // torch binary_cross_entropy_with_logits
    const float loss = (1.f - y) * x + mx + logf(expf(-mx) + expf(-x - mx));
    logp[r] = -loss;
  }
}

__global__ void bernoulli_bwd(const float* __restrict__ logit, const float* __restrict__ value,
                              const float* __restrict__ glogp, float* __restrict__ dlogit, long rows) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  dlogit[r] = glogp[r] * (value[r] - sigmoidf_(logit[r]));
}

// ---------------------------------------------------------------- Deter GRU-style gates (rssm.py:65-75)
// gates: (M, G, 3, Dg) = the dyn_gru BlockLinear output; h: (M, G*Dg)
__global__ void gru_fwd(const float* __restrict__ gates, const float* __restrict__ h, float* __restrict__ out, long M,
                        int G, int Dg) {
  const long D = (long)G * Dg;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= M * D) return;
  const long m = t / D;
  const int gd = (int)(t % D), g = gd / Dg, j = gd % Dg;
  const float* gr = gates + m * 3 * D + (long)g * 3 * Dg;
  const float rs = sigmoidf_(gr[j]);
  const float c = tanhf(rs * gr[Dg + j]);
  const float u = sigmoidf_(gr[2 * Dg + j] - 1.f);
  out[t] = u * c + (1.f - u) * h[t];
}

__global__ void gru_bwd(const float* __restrict__ gates, const float* __restrict__ h, const float* __restrict__ dout,
                        float* __restrict__ dgates, float* __restrict__ dh, long M, int G, int Dg, int accumulate_dh) {
  const long D = (long)G * Dg;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= M * D) return;
  const long m = t / D;
  const int gd = (int)(t % D), g = gd / Dg, j = gd % Dg;
  const long base = m * 3 * D + (long)g * 3 * Dg;
  const float ra = gates[base + j], ca = gates[base + Dg + j], ua = gates[base + 2 * Dg + j];
  const GruGrad gg = gru_gate_backward(ra, ca, ua, h[t], dout[t]);
  dgates[base + j] = gg.dr;
  dgates[base + Dg + j] = gg.dc;
  dgates[base + 2 * Dg + j] = gg.du;
  dh[t] = accumulate_dh ? dh[t] + gg.dh : gg.dh;
}

// ---------------------------------------------------------------- host side
// n work items (threads, one-wave rows, or whole blocks with per = 1), `per` of them per 256-thread block, on stream s
template <class Kern, class... Args>
int launch(Kern kern, long n, int per, sd_stream s, Args... args) {
  kern<<<sd_cdiv(n, per), 256, 0, (hipStream_t)s>>>(args...);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

// f(T) with the team width of a K-way categorical (the power of two in 8..64 that holds K) as an integral constant
template <class F>
int with_team(int K, F f) {
  if (K < 1 || K > 64) return SD_ESHAPE;
  if (K <= 8) return f(std::integral_constant<int, 8>());
  if (K <= 16) return f(std::integral_constant<int, 16>());
  if (K <= 32) return f(std::integral_constant<int, 32>());
  return f(std::integral_constant<int, 64>());
}

// bins of a two-hot row: one wave holds up to 256; the mode sums +- pairs around a centre bin (odd: 1..255)
bool twohot_bins_ok(int NB, bool odd = false) { return NB >= 1 && NB <= 256 && (!odd || NB % 2 == 1); }

}  // namespace

extern "C" int sd_onehot_sample_fwd(const float* logits, float* out, int* index, float* entropy, long groups, int K,
                                    float unimix, uint64_t seed, int stream_id, int step, long group_offset,
                                    const uint64_t* seed_ptr, sd_stream s) {
  if (groups <= 0) return SD_OK;
  return with_team(K, [&](auto T) {
    return launch(onehot_sample_fwd<T.value>, groups * T.value, 256, s, logits, out, index, entropy, groups, K, unimix,
                  seed, stream_id, step, group_offset, seed_ptr);
  });
}

extern "C" int sd_onehot_sample_bwd(const float* logits, const float* dout, float* dlogits, long groups, int K,
                                    float unimix, uint64_t seed, int stream_id, int step, long group_offset,
                                    int accumulate, const uint64_t* seed_ptr, sd_stream s) {
  if (groups <= 0) return SD_OK;
  return with_team(K, [&](auto T) {
    return launch(onehot_sample_bwd<T.value>, groups * T.value, 256, s, logits, dout, dlogits, groups, K, unimix, seed,
                  stream_id, step, group_offset, accumulate, seed_ptr);
  });
}

extern "C" int sd_onehot_logp_ent_fwd(const float* logits, const float* action, float* logp, float* ent, long rows,
                                      int K, float unimix, sd_stream s) {
  if (rows <= 0) return SD_OK;
  return with_team(K, [&](auto T) {
    return launch(onehot_logp_ent_fwd<T.value>, rows * T.value, 256, s, logits, action, logp, ent, rows, K, unimix);
  });
}

extern "C" int sd_onehot_logp_ent_bwd(const float* logits, const float* action, const float* glogp, const float* gent,
                                      float* dlogits, long rows, int K, float unimix, sd_stream s) {
  if (rows <= 0) return SD_OK;
  return with_team(K, [&](auto T) {
    return launch(onehot_logp_ent_bwd<T.value>, rows * T.value, 256, s, logits, action, glogp, gent, dlogits, rows, K,
                  unimix);
  });
}

extern "C" int sd_kl_fwd(const float* post, const float* prior, float* kl_row, float* dyn, float* rep, float free_nats,
                         int rows, int S, int K, sd_stream s) {
  if (rows <= 0) return SD_OK;
  return with_team(K, [&](auto T) {  // a block per row, grid-strided past 4096 rows
    return launch(kl_fwd<T.value>, rows < 4096 ? rows : 4096, 1, s, post, prior, kl_row, dyn, rep, free_nats, rows, S,
                  K);
  });
}

extern "C" int sd_kl_bwd(const float* post, const float* prior, const float* kl_row, const float* g_rep,
                         const float* g_dyn, float free_nats, float* d_post, float* d_prior, int rows, int S, int K,
                         int acc_post, int acc_prior, sd_stream s) {
  if (rows <= 0) return SD_OK;
  return with_team(K, [&](auto T) {
    return launch(kl_bwd<T.value>, (long)rows * S * T.value, 256, s, post, prior, kl_row, g_rep, g_dyn, free_nats,
                  d_post, d_prior, rows, S, K, acc_post, acc_prior);
  });
}

extern "C" int sd_twohot_mode(const float* logits, const float* bins, float* out, long rows, int NB, sd_stream s) {
  if (rows <= 0) return SD_OK;
  if (!twohot_bins_ok(NB, true)) return SD_ESHAPE;
  return launch(twohot_mode_kernel, rows, 4, s, logits, bins, out, rows, NB);
}

extern "C" int sd_twohot_mode_bwd(const float* logits, const float* bins, const float* dout, float* dlogits, long rows,
                                  int NB, sd_stream s) {
  if (rows <= 0) return SD_OK;
  if (!twohot_bins_ok(NB, true)) return SD_ESHAPE;
  return launch(twohot_mode_bwd_kernel, rows, 4, s, logits, bins, dout, dlogits, rows, NB);
}

extern "C" int sd_twohot_logp_fwd(const float* logits, const float* bins, const float* target, float* logp, long rows,
                                  int NB, sd_stream s) {
  if (rows <= 0) return SD_OK;
  if (!twohot_bins_ok(NB)) return SD_ESHAPE;
  return launch(twohot_logp_fwd, rows, 4, s, logits, bins, target, logp, rows, NB);
}

extern "C" int sd_twohot_logp_bwd(const float* logits, const float* bins, const float* target, const float* glogp,
                                  float* dlogits, long rows, int NB, int accumulate, sd_stream s) {
  if (rows <= 0) return SD_OK;
  if (!twohot_bins_ok(NB)) return SD_ESHAPE;
  return launch(twohot_logp_bwd, rows, 4, s, logits, bins, target, glogp, dlogits, rows, NB, accumulate);
}

extern "C" int sd_repval_loss_fwd(const float* logits, const float* bins, const float* ret, const float* slow,
                                  const float* last, float* row_loss, int B, int Tl, int Tr, int NB, sd_stream s) {
  if (B <= 0 || Tr <= 0) return SD_OK;
  if (!twohot_bins_ok(NB) || Tr > Tl) return SD_ESHAPE;
  return launch(repval_fwd_kernel, (long)B * Tr, 4, s, logits, bins, ret, slow, last, row_loss, (long)B * Tr, Tl, Tr,
                NB);
}

extern "C" int sd_repval_loss_bwd(const float* logits, const float* bins, const float* ret, const float* slow,
                                  const float* last, const float* gscale, float inv_n, float* dlogits, int B, int Tl,
                                  int Tr, int NB, sd_stream s) {
  if (B <= 0) return SD_OK;
  if (!twohot_bins_ok(NB) || !gscale || Tr > Tl) return SD_ESHAPE;
  return launch(repval_bwd_kernel, (long)B * Tl, 4, s, logits, bins, ret, slow, last, gscale, inv_n, dlogits,
                (long)B * Tl, Tl, Tr, NB);
}

extern "C" int sd_imag_ac_loss_fwd(const float* vl, const float* bins, const float* ret, const float* slow,
                                   const float* w, const float* val, const float* scale, const float* logpi,
                                   const float* ent, float coef, long N, int H, int H1, int NB, float* rows_v,
                                   float* rows_p, float* adv, sd_stream s) {
  if (N <= 0 || H <= 0) return SD_OK;
  if (!twohot_bins_ok(NB) || H1 <= H) return SD_ESHAPE;
  return launch(imag_ac_fwd_kernel, N * H, 4, s, vl, bins, ret, slow, w, val, scale, logpi, ent, coef, N, H, H1, NB,
                rows_v, rows_p, adv);
}

extern "C" int sd_imag_ac_loss_bwd(const float* vl, const float* bins, const float* ret, const float* slow,
                                   const float* w, const float* adv, const float* gpolicy, const float* gvalue,
                                   float spolicy, float svalue, float coef, long N, int H, int H1, int NB, float* dvl,
                                   float* dlogpi, float* dent, sd_stream s) {
  if (N <= 0 || H <= 0) return SD_OK;
  if (!twohot_bins_ok(NB) || H1 <= H) return SD_ESHAPE;
  return launch(imag_ac_bwd_kernel, N * H, 4, s, vl, bins, ret, slow, w, adv, gpolicy, gvalue, spolicy, svalue, coef,
                1.f / (float)(N * H), N, H, H1, NB, dvl, dlogpi, dent);
}

extern "C" int sd_bnormal_sample(const float* x, float* action, long rows, int A, float min_std, float max_std,
                                 uint64_t seed, int stream_id, int step, long row_offset, const uint64_t* seed_ptr,
                                 sd_stream s) {
  if (rows <= 0 || A <= 0) return SD_OK;
  return launch(bnormal_sample, rows * A, 256, s, x, action, rows, A, min_std, max_std, seed, stream_id, step,
                row_offset, seed_ptr);
}

extern "C" int sd_bnormal_sample_bwd(const float* d_action_norm, const float* x, const float* action, float* dx,
                                     long rows, int A, float min_std, float max_std, uint64_t seed, int stream_id,
                                     int step, long row_offset, const uint64_t* seed_ptr, sd_stream s) {
  if (rows <= 0 || A <= 0) return SD_OK;
  return launch(bnormal_sample_bwd, rows * A, 256, s, d_action_norm, x, action, dx, rows, A, min_std, max_std, seed,
                stream_id, step, row_offset, seed_ptr);
}

extern "C" int sd_bnormal_logp_ent_fwd(const float* x, const float* action, float* logp, float* ent, long rows, int A,
                                       float min_std, float max_std, sd_stream s) {
  if (rows <= 0 || A <= 0) return SD_OK;
  return launch(bnormal_logp_ent_fwd, rows, 256, s, x, action, logp, ent, rows, A, min_std, max_std);
}

extern "C" int sd_bnormal_logp_ent_bwd(const float* x, const float* action, const float* glogp, const float* gent,
                                       float* dx, long rows, int A, float min_std, float max_std, sd_stream s) {
  if (rows <= 0 || A <= 0) return SD_OK;
  return launch(bnormal_logp_ent_bwd, rows * A, 256, s, x, action, glogp, gent, dx, rows, A, min_std, max_std);
}

extern "C" int sd_bernoulli_fwd(const float* logit, const float* value, float* logp, float* mean, long rows,
                                sd_stream s) {
  if (rows <= 0) return SD_OK;
  return launch(bernoulli_fwd, rows, 256, s, logit, value, logp, mean, rows);
}

extern "C" int sd_bernoulli_bwd(const float* logit, const float* value, const float* glogp, float* dlogit, long rows,
                                sd_stream s) {
  if (rows <= 0) return SD_OK;
  return launch(bernoulli_bwd, rows, 256, s, logit, value, glogp, dlogit, rows);
}

extern "C" int sd_gru_fwd(const float* gates, const float* h, float* out, long M, int G, int Dg, sd_stream s) {
  if (M <= 0) return SD_OK;
  return launch(gru_fwd, M * G * Dg, 256, s, gates, h, out, M, G, Dg);
}

extern "C" int sd_gru_bwd(const float* gates, const float* h, const float* dout, float* dgates, float* dh, long M, int G,
                          int Dg, int accumulate_dh, sd_stream s) {
  if (M <= 0) return SD_OK;
  return launch(gru_bwd, M * G * Dg, 256, s, gates, h, dout, dgates, dh, M, G, Dg, accumulate_dh);
}
