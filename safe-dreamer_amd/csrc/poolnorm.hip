// The ConvEncoder layer tail as row kernels: MaxPool2d(2) -> RMSNorm2D -> SiLU over an NHWC conv output
// (networks.py:211-214), its backward, and the FiLM parameter gradients of the multimodal encoder. One team of T lanes
// per pooled pixel, VPT channels per lane; every entry goes through one forward and one backward launcher below.
// The fused conv + pool forward and the contractions that consume these gradients are in conv.hip.
#include <limits.h>

#include "sdhip.h"
#include "stage_core.h"

namespace {
// y = silu(rms(maxpool2(x))) per output pixel (team of T lanes, VPT channels each); keeps pooled + argmax.
template <int T, int VPT, class NW = const float* __restrict__>
__global__ void pool_rms_fwd(const float* __restrict__ x, NW w, float* __restrict__ pooled,
                             uint8_t* __restrict__ amax, float* __restrict__ y, float* __restrict__ rstd, int Nb, int H,
                             int W, int C, float eps, int nchw_flat) {
  const int Ho = H / 2, Wo = W / 2;
  const long P = (long)Nb * Ho * Wo;
  const long pix = ((long)blockIdx.x * blockDim.x + threadIdx.x) / T;
  const int t = threadIdx.x % T;
  if (pix >= P) return;
  const int n = (int)(pix / (Ho * Wo));
  const int rem = (int)(pix % (Ho * Wo));
  const int yo = rem / Wo, xo = rem % Wo;
  float v[VPT];
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int c = t + j * T;
    v[j] = 0.f;
    if (c < C) {
      float best = -INFINITY;
      int bi = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int yy = 2 * yo + (q >> 1), xx = 2 * xo + (q & 1);
        const float val = x[(((long)n * H + yy) * W + xx) * C + c];
        if (val > best || isnan(val)) { best = val; bi = q; }
      }
      v[j] = best;
      pooled[pix * C + c] = best;
      amax[pix * C + c] = (uint8_t)bi;
    }
    ss += v[j] * v[j];
  }
  ss = group_sum<T>(ss);
  const float r = rsqrtf(ss / (float)C + eps);
  if (t == 0) rstd[pix] = r;
  long fo = 0;
  if constexpr (is_film<NW>) fo = (long)(n / w.ipc) * C;
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int c = t + j * T;
    if (c < C) {
      float z = v[j] * r * nw_of(w)[c];
      if constexpr (is_film<NW>) z = w.gamma[fo + c] * z + w.beta[fo + c];
      const long o = nchw_flat ? (long)n * C * Ho * Wo + (long)c * Ho * Wo + rem : pix * C + c;
      y[o] = siluf_(z);
    }
  }
}

// COMPACT: dx is the pooled-resolution gradient (Nb, H/2, W/2, C) for sd_conv2d_wgrad_pool (no window scatter)
// FiLM (NW = FilmNW): z = gamma * norm + beta is recomputed, the gradient continues as dnorm = dz * gamma (the norm
// weight's partials are then sums of dz * gamma * xhat); dgamma / dbeta come from film_grad_partial below.
template <int T, int VPT, bool COMPACT = false, class NW = const float* __restrict__>
__global__ void pool_rms_bwd(const float* __restrict__ pooled, const uint8_t* __restrict__ amax,
                             NW w, const float* __restrict__ rstd, const float* __restrict__ dy,
                             float* __restrict__ dx, float* __restrict__ dw_part, int Nb, int H, int W, int C,
                             int nchw_flat) {
  const int Ho = H / 2, Wo = W / 2;
  const long P = (long)Nb * Ho * Wo;
  const int t = threadIdx.x % T;
  const int team = threadIdx.x / T;
  constexpr int TPB = 256 / T;
  float dwacc[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) dwacc[j] = 0.f;
  for (long pix = (long)blockIdx.x * TPB + team; pix < P; pix += (long)gridDim.x * TPB) {
    const int n = (int)(pix / (Ho * Wo));
    const int rem = (int)(pix % (Ho * Wo));
    const int yo = rem / Wo, xo = rem % Wo;
    const float r = rstd[pix];
    float xh[VPT], g[VPT];
    float dot = 0.f;
    long fo = 0;
    if constexpr (is_film<NW>) fo = (long)(n / w.ipc) * C;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int c = t + j * T;
      xh[j] = g[j] = 0.f;
      if (c < C) {
        const float xv = pooled[pix * C + c] * r;
        const float wv = nw_of(w)[c];
        float z = xv * wv;
        if constexpr (is_film<NW>) z = w.gamma[fo + c] * z + w.beta[fo + c];
        const float s = sigmoidf_(z);
        const long o = nchw_flat ? (long)n * C * Ho * Wo + (long)c * Ho * Wo + rem : pix * C + c;
        float dz = dy[o] * s * (1.f + z * (1.f - s));
        if constexpr (is_film<NW>) dz *= w.gamma[fo + c];
        xh[j] = xv;
        g[j] = dz * wv;
        dwacc[j] += dz * xv;
        dot += g[j] * xv;
      }
    }
    dot = group_sum<T>(dot) / (float)C;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int c = t + j * T;
      if (c < C) {
        const float dp = r * (g[j] - xh[j] * dot);
        if constexpr (COMPACT) {
          dx[pix * C + c] = dp;
        } else {
          const int bi = amax[pix * C + c];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int yy = 2 * yo + (q >> 1), xx = 2 * xo + (q & 1);
            dx[(((long)n * H + yy) * W + xx) * C + c] = q == bi ? dp : 0.f;
          }
          // an odd H or W: MaxPool2d(2) floors, so the last row / column belongs to no window and its gradient is
          // zero. The windows at the edge write it (dx is not cleared beforehand); even sizes take neither branch.
          const bool ex = (W & 1) && xo == Wo - 1, ey = (H & 1) && yo == Ho - 1;
          if (ex) {
            dx[(((long)n * H + 2 * yo) * W + W - 1) * C + c] = 0.f;
            dx[(((long)n * H + 2 * yo + 1) * W + W - 1) * C + c] = 0.f;
          }
          if (ey) {
            dx[(((long)n * H + H - 1) * W + 2 * xo) * C + c] = 0.f;
            dx[(((long)n * H + H - 1) * W + 2 * xo + 1) * C + c] = 0.f;
            if (ex) dx[(((long)n * H + H - 1) * W + W - 1) * C + c] = 0.f;
          }
        }
      }
    }
  }
  // per-block dw partials
  __shared__ float wp[TPB * T * VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) wp[(team * VPT + j) * T + t] = dwacc[j];
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    const int j = c / T, tt = c % T;
    float s = 0.f;
    for (int tm = 0; tm < TPB; ++tm) s += wp[(tm * VPT + j) * T + tt];
    dw_part[(long)blockIdx.x * C + c] = s;
  }
}

// FiLM parameter gradients of a stage, first pass: workgroup (blk, b) walks context row b's ipc * Ho * Wo pooled pixels
// (16 teams of 16 lanes, VPT channels per lane, as pool_rms_bwd), recomputes dz = dy * silu'(gamma * norm + beta) and
// keeps S0 = sum dz, S1 = sum dz * xhat per channel; the 16 teams are added in team order and the block's sums go to
// part[b][blk][2][C]. film_grad_final adds the blocks in block order: dbeta = S0, dgamma = nw * S1 (norm = xhat * nw).
// No atomics: the result does not depend on the schedule.
template <int T, int VPT>
__global__ __launch_bounds__(256) void film_grad_partial(const float* __restrict__ pooled, const FilmNW w,
                                                         const float* __restrict__ rstd,
                                                         const float* __restrict__ dy, float* __restrict__ part,
                                                         int Ho, int Wo, int C, int nchw_flat) {
  const int t = threadIdx.x % T, team = threadIdx.x / T, b = blockIdx.y;
  constexpr int TPB = 256 / T;
  const int hw = Ho * Wo;
  const long rowpix = (long)w.ipc * hw, pix0 = (long)b * rowpix;
  float s0[VPT], s1[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) s0[j] = s1[j] = 0.f;
  for (long lp = (long)blockIdx.x * TPB + team; lp < rowpix; lp += (long)gridDim.x * TPB) {
    const long pix = pix0 + lp;
    const int n = (int)(pix / hw), rem = (int)(pix % hw);
    const float r = rstd[pix];
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int c = t + j * T;
      if (c < C) {
        const float xv = pooled[pix * C + c] * r;
        const float z = w.gamma[(long)b * C + c] * (xv * w.nw[c]) + w.beta[(long)b * C + c];
        const float s = sigmoidf_(z);
        const long o = nchw_flat ? (long)n * C * hw + (long)c * hw + rem : pix * C + c;
        const float dz = dy[o] * s * (1.f + z * (1.f - s));
        s0[j] += dz;
        s1[j] += dz * xv;
      }
    }
  }
  __shared__ float sp[2][TPB * T * VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    sp[0][(team * VPT + j) * T + t] = s0[j];
    sp[1][(team * VPT + j) * T + t] = s1[j];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += 256) {
    const int k = i / C, c = i % C, j = c / T, tt = c % T;
    float s = 0.f;
    for (int tm = 0; tm < TPB; ++tm) s += sp[k][(tm * VPT + j) * T + tt];
    part[(((long)b * gridDim.x + blockIdx.x) * 2 + k) * C + c] = s;
  }
}

__global__ void film_grad_final(const float* __restrict__ part, const float* __restrict__ nw,
                                float* __restrict__ dgamma, float* __restrict__ dbeta, int rows, int nblk, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * C) return;
  const int b = i / C, c = i % C;
  float s0 = 0.f, s1 = 0.f;
  for (int k = 0; k < nblk; ++k) {
    s0 += part[(((long)b * nblk + k) * 2 + 0) * C + c];
    s1 += part[(((long)b * nblk + k) * 2 + 1) * C + c];
  }
  dbeta[i] = s0;
  dgamma[i] = s1 * nw[c];
}

int vpt_for(int C, int T) { int v = (C + T - 1) / T; return v <= 1 ? 1 : v <= 2 ? 2 : v <= 4 ? 4 : 8; }

// ---------------------------------------------------------------- host side: one family description, two launchers
// A family of entries: T lanes per pooled pixel, so a 256-thread workgroup holds ppw = 256 / T pixels; the channel
// counts it admits (cmin <= C <= cmax); the channels per lane its kernels are instantiated for. Narrow: 16 teams of 16
// lanes, 1 / 2 / 4 / 8 channels per lane. Wide: a whole wave per pixel, 4 or 8 channels per lane, the same kernels line
// for line (ss and dot summed over the 64 lanes). Each refuses the other's C before anything else: nothing launched, no
// pointer read. A launcher names only its own family's (T, VPT) pairs, so no kernel exists that no entry can reach.
template <int T_, int CMIN, int CMAX, int... VPTS>
struct Family {
  static constexpr int T = T_, ppw = 256 / T_;
  static bool admits(int C) { return C >= CMIN && C <= CMAX; }
  // f(VPT as an integral constant) for the channels per lane that cover C
  template <class F>
  static void with_vpt(int C, F&& f) { with_int<VPTS...>(vpt_for(C, T), f); }
};
using Narrow = Family<16, INT_MIN, 128, 1, 2, 4, 8>;
using Wide = Family<64, 129, SD_POOL_WIDE_MAX, 4, 8>;
constexpr int BWD_BLOCKS_MAX = 2048, FILM_BLOCKS_MAX = 64;

long pooled_pixels(int images, int H, int W) { return (long)images * (H / 2) * (W / 2); }

// workgroups of a grid-stride kernel over `pixels` pooled pixels: one per ppw pixels, in [1, cap]
int row_blocks(int ppw, long pixels, int cap) {
  const long b = (pixels + ppw - 1) / ppw;
  return (int)(b < cap ? (b > 0 ? b : 1) : cap);
}
int film_floats(int ppw, int Nb, int ipc, int H, int W, int C) {
  if (ipc <= 0) return 0;
  return (Nb / ipc) * row_blocks(ppw, pooled_pixels(ipc, H, W), FILM_BLOCKS_MAX) * 2 * C;
}

template <class Fam, class NW>
int pool_fwd(const float* x, NW w, float* pooled, uint8_t* amax, float* y, float* rstd, int Nb, int H, int W, int C,
             float eps, int nchw_flat, sd_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (!Fam::admits(C)) return SD_ESHAPE;
  if constexpr (is_film<NW>) {
    if (!w.gamma || !w.beta || w.ipc <= 0 || Nb % w.ipc) return SD_EARG;
  }
  const long P = pooled_pixels(Nb, H, W);
  if (P <= 0) return SD_OK;
  const long grid = (P + Fam::ppw - 1) / Fam::ppw;
  if (grid > 0x7fffffffL) return SD_ESHAPE;
  Fam::with_vpt(C, [&](auto V) {
    pool_rms_fwd<Fam::T, V(), NW><<<(int)grid, 256, 0, s>>>(x, w, pooled, amax, y, rstd, Nb, H, W, C, eps, nchw_flat);
  });
  SD_LAUNCH_CHECK();
  return SD_OK;
}

// An image of one row or one column has no 2x2 window: the conv gradient is all zeros and no pooled pixel exists to
// write it (the degenerate case only; every other shape is written by the kernel itself, odd edges included).
int pool_rms_bwd_empty(float* dx, int Nb, int H, int W, int C, hipStream_t s) {
  const long n = (long)Nb * H * W * C;
  if (n <= 0 || ((H / 2) > 0 && (W / 2) > 0)) return SD_OK;
  return hipMemsetAsync(dx, 0, (size_t)n * sizeof(float), s) == hipSuccess ? SD_OK : SD_EARG;
}

// the FiLM backward's outputs: dgamma, dbeta (rows, C), overwritten, and >= film_floats floats of partials
struct FilmGrad {
  float *dgamma, *dbeta, *partial;
};

// dx: the scattered conv gradient, or with COMPACT the pooled-resolution one for sd_conv2d_wgrad_pool (narrow only).
// dw by the two-pass column sum of the per-block partials; its chunk workspace follows them in dw_partial.
// FiLM: dnorm through gamma in the main kernel, then dgamma / dbeta by film_grad_partial + film_grad_final.
template <class Fam, bool COMPACT, class NW>
int pool_bwd(const float* pooled, const uint8_t* amax, NW w, const float* rstd, const float* dy, float* dx, float* dw,
             float* dw_partial, FilmGrad fg, int Nb, int H, int W, int C, int nchw_flat, int accumulate_dw,
             sd_stream stream_) {
  static_assert(!COMPACT || Fam::T == 16, "there is no wide compact backward");
  hipStream_t s = (hipStream_t)stream_;
  if (!Fam::admits(C)) return SD_ESHAPE;
  if constexpr (is_film<NW>) {
    if (!w.gamma || !w.beta || !fg.dgamma || !fg.dbeta || !fg.partial || w.ipc <= 0 || Nb % w.ipc) return SD_EARG;
    if (Nb <= 0) return SD_OK;
  }
  const int grid = row_blocks(Fam::ppw, pooled_pixels(Nb, H, W), BWD_BLOCKS_MAX);
  if (!COMPACT && pool_rms_bwd_empty(dx, Nb, H, W, C, s) != SD_OK) return SD_EARG;
  Fam::with_vpt(C, [&](auto V) {
    pool_rms_bwd<Fam::T, V(), COMPACT, NW><<<grid, 256, 0, s>>>(pooled, amax, w, rstd, dy, dx, dw_partial, Nb, H, W, C,
                                                                 nchw_flat);
  });
  SD_LAUNCH_CHECK();
  if constexpr (is_film<NW>) {
    const int rows = Nb / w.ipc, nblk = row_blocks(Fam::ppw, pooled_pixels(w.ipc, H, W), FILM_BLOCKS_MAX);
    Fam::with_vpt(C, [&](auto V) {
      film_grad_partial<Fam::T, V()><<<dim3(nblk, rows), 256, 0, s>>>(pooled, w, rstd, dy, fg.partial, H / 2, W / 2, C,
                                                                       nchw_flat);
    });
    SD_LAUNCH_CHECK();
    film_grad_final<<<sd_cdiv((long)rows * C, 256), 256, 0, s>>>(fg.partial, w.nw, fg.dgamma, fg.dbeta, rows, nblk, C);
    SD_LAUNCH_CHECK();
  }
  return sd_colsum_ws(dw_partial, dw, grid, C, C, accumulate_dw, dw_partial + (long)grid * C, stream_);
}
}  // namespace

extern "C" int sd_pool_rms_fwd(const float* x, const float* w, float* pooled, uint8_t* amax, float* y, float* rstd,
                               int Nb, int H, int W, int C, float eps, int nchw_flat, sd_stream stream_) {
  return pool_fwd<Narrow>(x, w, pooled, amax, y, rstd, Nb, H, W, C, eps, nchw_flat, stream_);
}

extern "C" int sd_pool_rms_fwd_film(const float* x, const float* w, const float* gamma, const float* beta, int ipc,
                                    float* pooled, uint8_t* amax, float* y, float* rstd, int Nb, int H, int W, int C,
                                    float eps, int nchw_flat, sd_stream stream_) {
  return pool_fwd<Narrow>(x, FilmNW{w, gamma, beta, ipc}, pooled, amax, y, rstd, Nb, H, W, C, eps, nchw_flat, stream_);
}

extern "C" int sd_pool_rms_wide_fwd(const float* x, const float* w, float* pooled, uint8_t* amax, float* y,
                                    float* rstd, int Nb, int H, int W, int C, float eps, int nchw_flat,
                                    sd_stream stream_) {
  return pool_fwd<Wide>(x, w, pooled, amax, y, rstd, Nb, H, W, C, eps, nchw_flat, stream_);
}

extern "C" int sd_pool_rms_wide_fwd_film(const float* x, const float* w, const float* gamma, const float* beta,
                                         int ipc, float* pooled, uint8_t* amax, float* y, float* rstd, int Nb, int H,
                                         int W, int C, float eps, int nchw_flat, sd_stream stream_) {
  return pool_fwd<Wide>(x, FilmNW{w, gamma, beta, ipc}, pooled, amax, y, rstd, Nb, H, W, C, eps, nchw_flat, stream_);
}

extern "C" int sd_pool_rms_bwd_blocks(int Nb, int H, int W) {
  return row_blocks(Narrow::ppw, pooled_pixels(Nb, H, W), BWD_BLOCKS_MAX);
}
extern "C" int sd_pool_rms_wide_bwd_blocks(int Nb, int H, int W) {
  return row_blocks(Wide::ppw, pooled_pixels(Nb, H, W), BWD_BLOCKS_MAX);
}
extern "C" int sd_film_grad_floats(int Nb, int ipc, int H, int W, int C) {
  return film_floats(Narrow::ppw, Nb, ipc, H, W, C);
}
extern "C" int sd_film_grad_wide_floats(int Nb, int ipc, int H, int W, int C) {
  return film_floats(Wide::ppw, Nb, ipc, H, W, C);
}

extern "C" int sd_pool_rms_bwd(const float* pooled, const uint8_t* amax, const float* w, const float* rstd,
                               const float* dy, float* dx, float* dw, float* dw_partial, int Nb, int H, int W, int C,
                               int nchw_flat, int accumulate_dw, sd_stream stream_) {
  return pool_bwd<Narrow, false>(pooled, amax, w, rstd, dy, dx, dw, dw_partial, {}, Nb, H, W, C, nchw_flat,
                                  accumulate_dw, stream_);
}

extern "C" int sd_pool_rms_bwd_compact(const float* pooled, const uint8_t* amax, const float* w, const float* rstd,
                                       const float* dy, float* dpool, float* dw, float* dw_partial, int Nb, int H,
                                       int W, int C, int nchw_flat, int accumulate_dw, sd_stream stream_) {
  return pool_bwd<Narrow, true>(pooled, amax, w, rstd, dy, dpool, dw, dw_partial, {}, Nb, H, W, C, nchw_flat,
                                 accumulate_dw, stream_);
}

extern "C" int sd_pool_rms_wide_bwd(const float* pooled, const uint8_t* amax, const float* w, const float* rstd,
                                    const float* dy, float* dx, float* dw, float* dw_partial, int Nb, int H, int W,
                                    int C, int nchw_flat, int accumulate_dw, sd_stream stream_) {
  return pool_bwd<Wide, false>(pooled, amax, w, rstd, dy, dx, dw, dw_partial, {}, Nb, H, W, C, nchw_flat,
                                  accumulate_dw, stream_);
}

// FiLM backward: dgamma / dbeta (rows, C) overwritten; film_partial >= sd_film_grad[_wide]_floats floats.
extern "C" int sd_pool_rms_bwd_film(const float* pooled, const uint8_t* amax, const float* w, const float* gamma,
                                    const float* beta, int ipc, const float* rstd, const float* dy, float* dx,
                                    float* dw, float* dw_partial, float* dgamma, float* dbeta, float* film_partial,
                                    int Nb, int H, int W, int C, int nchw_flat, int accumulate_dw, sd_stream stream_) {
  return pool_bwd<Narrow, false>(pooled, amax, FilmNW{w, gamma, beta, ipc}, rstd, dy, dx, dw, dw_partial,
                         {dgamma, dbeta, film_partial}, Nb, H, W, C, nchw_flat, accumulate_dw, stream_);
}

extern "C" int sd_pool_rms_bwd_compact_film(const float* pooled, const uint8_t* amax, const float* w,
                                            const float* gamma, const float* beta, int ipc, const float* rstd,
                                            const float* dy, float* dpool, float* dw, float* dw_partial, float* dgamma,
                                            float* dbeta, float* film_partial, int Nb, int H, int W, int C,
                                            int nchw_flat, int accumulate_dw, sd_stream stream_) {
  return pool_bwd<Narrow, true>(pooled, amax, FilmNW{w, gamma, beta, ipc}, rstd, dy, dpool, dw, dw_partial,
                        {dgamma, dbeta, film_partial}, Nb, H, W, C, nchw_flat, accumulate_dw, stream_);
}

extern "C" int sd_pool_rms_wide_bwd_film(const float* pooled, const uint8_t* amax, const float* w, const float* gamma,
                                         const float* beta, int ipc, const float* rstd, const float* dy, float* dx,
                                         float* dw, float* dw_partial, float* dgamma, float* dbeta,
                                         float* film_partial, int Nb, int H, int W, int C, int nchw_flat,
                                         int accumulate_dw, sd_stream stream_) {
  return pool_bwd<Wide, false>(pooled, amax, FilmNW{w, gamma, beta, ipc}, rstd, dy, dx, dw, dw_partial,
                         {dgamma, dbeta, film_partial}, Nb, H, W, C, nchw_flat, accumulate_dw, stream_);
}
