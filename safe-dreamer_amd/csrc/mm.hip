// Text-conditioned (multimodal) encoder pieces outside the conv stages: the per-context-row bias + SiLU of the gate
// and FiLM MLPs, the text gate's mixture and the attention pooling of the frozen text token features.
// Every sum over the T rows of a context row runs in one thread in row order (no atomics: results do not depend on
// the schedule, so a graph replay equals the eager run bit for bit).
#include "common.h"
#include "sdhip.h"

namespace {

// exact-division sigmoid: the gate value is a reported diagnostic and feeds the posterior's input
SD_DEV float sigmoid_exact(float x) { return 1.f / (1.f + expf(-x)); }

// y[n][e] = silu(x[n][e] + u[n / T][e]); u == nullptr: y = silu(x)
__global__ __launch_bounds__(256) void rowbias_silu_fwd(const float* __restrict__ x, const float* __restrict__ u,
                                                        float* __restrict__ y, long total, int E, int T) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float z = x[i];
  if (u) {
    const long n = i / E;
    z += u[(n / T) * E + (i - n * E)];
  }
  y[i] = siluf_(z);
}

// dx[n][e] = dy * silu'(x + u[n / T]); du[b][e] = sum over the T rows of b of dx, in row order. Thread (b, e).
__global__ __launch_bounds__(64) void rowbias_silu_bwd(const float* __restrict__ x, const float* __restrict__ u,
                                                       const float* __restrict__ dy, float* __restrict__ dx,
                                                       float* __restrict__ du, int E, int T) {
  const int e = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
  if (e >= E) return;
  const float uv = u ? u[(long)b * E + e] : 0.f;
  float acc = 0.f;
  for (int t = 0; t < T; ++t) {
    const long i = ((long)b * T + t) * E + e;
    const float z = x[i] + uv;
    const float s = sigmoidf_(z);
    const float d = dy[i] * s * (1.f + z * (1.f - s));
    dx[i] = d;
    acc += d;
  }
  if (du) du[(long)b * E + e] = acc;
}

// g = sigmoid(a); out = v + g * (tp[n / T] - v)   (= (1 - g) v + g tp)
__global__ __launch_bounds__(256) void text_gate_fwd(const float* __restrict__ v, const float* __restrict__ a,
                                                     const float* __restrict__ tp, float* __restrict__ out,
                                                     float* __restrict__ g, long total, int E, int T) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long n = i / E;
  const float vv = v[i], tv = tp[(n / T) * E + (i - n * E)];
  const float gv = sigmoid_exact(a[i]);
  g[i] = gv;
  out[i] = vv + gv * (tv - vv);
}

// dv = (1 - g) d; da = d (tp - v) g (1 - g); dtp[b][e] = sum over the T rows of b of g d, in row order. Thread (b, e).
__global__ __launch_bounds__(64) void text_gate_bwd(const float* __restrict__ v, const float* __restrict__ g,
                                                    const float* __restrict__ tp, const float* __restrict__ d,
                                                    float* __restrict__ dv, float* __restrict__ da,
                                                    float* __restrict__ dtp, int E, int T) {
  const int e = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
  if (e >= E) return;
  const float tv = tp[(long)b * E + e];
  float acc = 0.f;
  for (int t = 0; t < T; ++t) {
    const long i = ((long)b * T + t) * E + e;
    const float gv = g[i], dd = d[i];
    dv[i] = (1.f - gv) * dd;
    da[i] = dd * (tv - v[i]) * gv * (1.f - gv);
    acc += gv * dd;
  }
  dtp[(long)b * E + e] = acc;
}

// Attention pooling of one text's token features (ntok <= 128 tokens, D channels): score = f . w + b, softmax over the
// tokens, out = sum p f. One 256-thread workgroup per text: a wave per token for the scores, a thread per channel
// for the weighted sum (tokens in order).
constexpr int MAX_TOK = 128;
__global__ __launch_bounds__(256) void text_pool(const float* __restrict__ f, const float* __restrict__ w,
                                                 const float* __restrict__ bias, float* __restrict__ out, int ntok,
                                                 int D) {
  __shared__ float sc[MAX_TOK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* fb = f + (long)blockIdx.x * ntok * D;
  for (int i = wave; i < ntok; i += 4) {
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += fb[(long)i * D + d] * w[d];
    s = wave_sum(s);
    if (lane == 0) sc[i] = s + bias[0];
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int i = 0; i < ntok; ++i) mx = fmaxf(mx, sc[i]);
  float den = 0.f;
  for (int i = 0; i < ntok; ++i) den += expf(sc[i] - mx);
  const float inv = 1.f / den;
  for (int d = threadIdx.x; d < D; d += 256) {
    float acc = 0.f;
    for (int i = 0; i < ntok; ++i) acc += expf(sc[i] - mx) * inv * fb[(long)i * D + d];
    out[(long)blockIdx.x * D + d] = acc;
  }
}

}  // namespace

extern "C" int sd_rowbias_silu_fwd(const float* x, const float* u, float* y, int N, int E, int T, sd_stream stream_) {
  if (N <= 0 || E <= 0) return SD_OK;
  if (u && (T <= 0 || N % T)) return SD_EARG;
  const long total = (long)N * E;
  rowbias_silu_fwd<<<sd_cdiv(total, 256), 256, 0, (hipStream_t)stream_>>>(x, u, y, total, E, u ? T : 1);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_rowbias_silu_bwd(const float* x, const float* u, const float* dy, float* dx, float* du, int N, int E,
                                   int T, sd_stream stream_) {
  if (N <= 0 || E <= 0) return SD_OK;
  if (T <= 0 || N % T) return SD_EARG;
  if (N / T > 65535) return SD_ESHAPE;
  rowbias_silu_bwd<<<dim3(sd_cdiv(E, 64), N / T), 64, 0, (hipStream_t)stream_>>>(x, u, dy, dx, du, E, T);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_text_gate_fwd(const float* v, const float* a, const float* tp, float* out, float* g, int N, int E,
                                int T, sd_stream stream_) {
  if (N <= 0 || E <= 0) return SD_OK;
  if (T <= 0 || N % T) return SD_EARG;
  const long total = (long)N * E;
  text_gate_fwd<<<sd_cdiv(total, 256), 256, 0, (hipStream_t)stream_>>>(v, a, tp, out, g, total, E, T);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_text_gate_bwd(const float* v, const float* g, const float* tp, const float* d, float* dv, float* da,
                                float* dtp, int N, int E, int T, sd_stream stream_) {
  if (N <= 0 || E <= 0) return SD_OK;
  if (T <= 0 || N % T) return SD_EARG;
  if (N / T > 65535) return SD_ESHAPE;
  text_gate_bwd<<<dim3(sd_cdiv(E, 64), N / T), 64, 0, (hipStream_t)stream_>>>(v, g, tp, d, dv, da, dtp, E, T);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_text_pool(const float* feats, const float* w, const float* bias, float* out, int ntexts, int ntok,
                            int D, sd_stream stream_) {
  if (ntexts <= 0) return SD_OK;
  if (ntok <= 0 || ntok > MAX_TOK || D <= 0) return SD_ESHAPE;
  text_pool<<<ntexts, 256, 0, (hipStream_t)stream_>>>(feats, w, bias, out, ntok, D);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
