// Adversarial image patch (sdreamer/attack.py): compositing, the patch gradient and the optimizer step.
//
//  * sd_patch_apply: the patch pasted into every image at a per-image top-left offset (clipped at the borders), the
//    f32 image and the encoder input (image - shift, channel-padded) written by the same launch;
//  * sd_patch_grad: the adjoint — each patch element's sum of the image gradient over the images whose clipped window
//    contains it, in two fixed-order stages (chunks of SD_PATCH_CHUNK images in image order, then the chunks in chunk
//    order), optionally + w_tv * d TV / d patch (anisotropic total variation) and the TV value;
//  * sd_patch_step: one Adam step (torch.optim.Adam's arithmetic), the projection onto [0, 1] and onto the L-inf ball
//    around a base patch; the step counter lives on the device.
// No atomics anywhere: the same inputs give the same bits.
#include "common.h"
#include "sdhip.h"

namespace {

template <bool U8>
__global__ void patch_apply_k(const void* __restrict__ in, const float* __restrict__ patch,
                              const int* __restrict__ offs, float* __restrict__ img, float* __restrict__ enc, long pixels,
                              int H, int W, int C, int Cp, int ph, int pw, float shift) {
  const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= pixels) return;
  const int x = (int)(pix % W);
  const long r = pix / W;
  const int y = (int)(r % H);
  const long n = r / H;
  const long py = (long)y - offs[2 * n], px = (long)x - offs[2 * n + 1];
  const bool inside = py >= 0 && py < ph && px >= 0 && px < pw;
  for (int c = 0; c < Cp; ++c) {
    float v = 0.f;
    if (c < C) {
      float f;
      if (inside) f = patch[(py * pw + px) * C + c];
      else if constexpr (U8) f = (float)static_cast<const uint8_t*>(in)[pix * C + c] / 255.0f;
      else f = static_cast<const float*>(in)[pix * C + c];
      if (img) img[pix * C + c] = f;
      v = f - shift;
    }
    if (enc) enc[pix * Cp + c] = v;
  }
}

// part[k][e] = sum over the images of chunk k (image order) of d_image at patch element e's position
__global__ void patch_grad_part_k(const float* __restrict__ dimg, const int* __restrict__ offs,
                                  float* __restrict__ part, int Nb, int H, int W, int C, int ph, int pw) {
  const int E = ph * pw * C;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int c = e % C, px = (e / C) % pw, py = e / (C * pw);
  const int n0 = blockIdx.y * SD_PATCH_CHUNK, n1 = min(Nb, n0 + SD_PATCH_CHUNK);
  float s = 0.f;
  for (int n = n0; n < n1; ++n) {
    const long y = (long)offs[2 * n] + py, x = (long)offs[2 * n + 1] + px;
    if (y >= 0 && y < H && x >= 0 && x < W) s += dimg[(((long)n * H + y) * W + x) * C + c];
  }
  part[(long)blockIdx.y * E + e] = s;
}

SD_DEV float sgnf_(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// one workgroup: dpatch[e] = sum_k part[k][e] (+ w_tv * dTV/dp[e]); tv[0] = TV(patch)
__global__ __launch_bounds__(256) void patch_grad_final_k(const float* __restrict__ part, int chunks,
                                                          const float* __restrict__ patch, float w_tv,
                                                          float* __restrict__ dpatch, float* __restrict__ tv, int C,
                                                          int ph, int pw) {
  __shared__ float red[4];
  const int E = ph * pw * C;
  float tvs = 0.f;
  for (int e = threadIdx.x; e < E; e += 256) {
    float s = 0.f;
    for (int k = 0; k < chunks; ++k) s += part[(long)k * E + e];
    if (patch) {
      const int px = (e / C) % pw, py = e / (C * pw);
      const float p = patch[e];
      float g = 0.f;
      if (px + 1 < pw) {
        const float d = patch[e + C] - p;
        tvs += fabsf(d);
        g -= sgnf_(d);
      }
      if (px > 0) g += sgnf_(p - patch[e - C]);
      if (py + 1 < ph) {
        const float d = patch[e + pw * C] - p;
        tvs += fabsf(d);
        g -= sgnf_(d);
      }
      if (py > 0) g += sgnf_(p - patch[e - pw * C]);
      s += w_tv * g;
    }
    dpatch[e] = s;
  }
  tvs = block_sum<256>(tvs, red);
  if (tv && threadIdx.x == 0) tv[0] = tvs;
}

// one workgroup (the step counter is read by every thread before thread 0 advances it)
__global__ __launch_bounds__(256) void patch_step_k(float* __restrict__ patch, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v,
                                                    int* __restrict__ step, const float* __restrict__ base, float lr,
                                                    float b1, float b2, float adam_eps, float linf, int n) {
  const int t = step[0] + 1;
  __syncthreads();
  if (threadIdx.x == 0) step[0] = t;
  const double bc1 = 1.0 - pow((double)b1, (double)t), bc2 = 1.0 - pow((double)b2, (double)t);
  const float step_size = (float)((double)lr / bc1), bc2s = (float)sqrt(bc2);
  for (int i = threadIdx.x; i < n; i += 256) {
    const float gi = g[i];
    const float mi = m[i] + (gi - m[i]) * (1.f - b1);  // torch: exp_avg.lerp_(grad, 1 - beta1)
    const float vi = v[i] * b2 + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2s + adam_eps;
    float p = patch[i] - step_size * (mi / denom);
    p = fminf(fmaxf(p, 0.f), 1.f);
    if (base) p = fminf(fmaxf(p, base[i] - linf), base[i] + linf);
    patch[i] = p;
  }
}

}  // namespace

extern "C" int sd_patch_apply(const void* in, int in_u8, const float* patch, const int* offsets, float* img,
                              float* enc, int Nb, int H, int W, int C, int Cp, int ph, int pw, float shift,
                              sd_stream stream_) {
  if (Nb <= 0) return SD_OK;
  if (!in || !patch || !offsets || (!img && !enc) || H <= 0 || W <= 0 || C <= 0 || Cp < C || ph <= 0 || pw <= 0)
    return SD_EARG;
  const long pixels = (long)Nb * H * W;
  hipStream_t s = (hipStream_t)stream_;
  if (in_u8)
    patch_apply_k<true><<<sd_cdiv(pixels, 256), 256, 0, s>>>(in, patch, offsets, img, enc, pixels, H, W, C, Cp, ph, pw,
                                                            shift);
  else
    patch_apply_k<false><<<sd_cdiv(pixels, 256), 256, 0, s>>>(in, patch, offsets, img, enc, pixels, H, W, C, Cp, ph,
                                                             pw, shift);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_patch_grad(const float* dimg, const int* offsets, float* dpatch, float* part, long part_floats,
                             const float* patch, float w_tv, float* tv, int Nb, int H, int W, int C, int ph, int pw,
                             sd_stream stream_) {
  if (!dimg || !offsets || !dpatch || !part || Nb <= 0 || H <= 0 || W <= 0 || C <= 0 || ph <= 0 || pw <= 0)
    return SD_EARG;
  const int E = ph * pw * C, chunks = sd_cdiv(Nb, SD_PATCH_CHUNK);
  if (part_floats < (long)chunks * E || chunks > 65535) return SD_EARG;
  hipStream_t s = (hipStream_t)stream_;
  patch_grad_part_k<<<dim3(sd_cdiv(E, 256), chunks), 256, 0, s>>>(dimg, offsets, part, Nb, H, W, C, ph, pw);
  SD_LAUNCH_CHECK();
  patch_grad_final_k<<<1, 256, 0, s>>>(part, chunks, patch, w_tv, dpatch, tv, C, ph, pw);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_patch_step(float* patch, const float* dpatch, float* m, float* v, int* step, const float* base,
                             float lr, float beta1, float beta2, float adam_eps, float linf_eps, long n,
                             sd_stream stream_) {
  if (!patch || !dpatch || !m || !v || !step || n <= 0 || n > 0x7fffffffL || (base && linf_eps < 0.f)) return SD_EARG;
  patch_step_k<<<1, 256, 0, (hipStream_t)stream_>>>(patch, dpatch, m, v, step, base, lr, beta1, beta2, adam_eps,
                                                    linf_eps, (int)n);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
