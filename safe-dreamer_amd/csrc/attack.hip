// Adversarial image patch (sdreamer/attack.py): compositing, the patch gradient and the optimizer step.
//
//  * sd_patch_apply: the patch pasted into every image at a per-image top-left offset (clipped at the borders), the
//    f32 image and the encoder input (image - shift, channel-padded) written by the same launch;
//  * sd_patch_grad: the adjoint — each patch element's sum of the image gradient over the images whose clipped window
//    contains it, in two fixed-order stages (chunks of SD_PATCH_CHUNK images in image order, then the chunks in chunk
//    order), optionally + w_tv * d TV / d patch (anisotropic total variation) and the TV value;
//  * sd_patch_apply_affine / sd_patch_grad_affine: the same pair with the patch resampled bilinearly through a
//    per-image affine map and a gain / bias (expectation over transformations: scale, rotation, sub-pixel placement,
//    contrast, brightness); the row layout is in sdhip.h, the host builds the rows (attack.transform_rows);
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

// ---- the resampling compositor (sd_patch_apply_affine / sd_patch_grad_affine). One tf row per image maps a pixel
// centre to continuous patch coordinates; the forward and its adjoint form the coordinates, the fractions and the
// bilinear weights through the functions below, so the two kernels are adjoint to rounding.
struct PatchTf {
  float a00, a01, b0, a10, a11, b1, gain, off;  // P(p) = clamp(gain * p + off, 0, 1), off = 0.5 - 0.5 gain + bias
};

SD_DEV PatchTf patch_tf_row(const float* __restrict__ tf, long n) {
  const float* r = tf + n * SD_PATCH_TF;
  // gain * p + off is gain * (p - 0.5) + 0.5 + bias with the constants gathered: gain 1, bias 0 gives off = 0 and
  // P(p) = p exactly for every p in [0, 1] (p - 0.5 + 0.5 would round p below 0.25)
  return {r[0], r[1], r[2], r[3], r[4], r[5], r[6], (0.5f - 0.5f * r[6]) + r[7]};
}

// (i0, j0) = the upper-left tap of pixel (y, x), (fu, fv) its fractions; false: no tap can lie in the patch (also for
// a non-finite coordinate), and nothing else is written
SD_DEV bool patch_coords(const PatchTf& t, int y, int x, int ph, int pw, int& i0, int& j0, float& fu, float& fv) {
  const float u = fmaf(t.a00, (float)y, fmaf(t.a01, (float)x, t.b0));
  const float v = fmaf(t.a10, (float)y, fmaf(t.a11, (float)x, t.b1));
  if (!(u > -1.f && u < (float)ph && v > -1.f && v < (float)pw)) return false;
  const float ufl = floorf(u), vfl = floorf(v);
  i0 = (int)ufl, j0 = (int)vfl, fu = u - ufl, fv = v - vfl;
  return true;
}

// weight of tap (i0 + di, j0 + dj), di, dj in {0, 1}
SD_DEV float patch_tap_weight(int di, int dj, float fu, float fv) {
  return (di ? fu : 1.f - fu) * (dj ? fv : 1.f - fv);
}

// one channel of one pixel: the input f blended with the resampled patch (alpha == 0: f itself, as
// sd_u8_image_inputs forms it; alpha == 1: q exactly)
SD_DEV float patch_blend(const PatchTf& t, const float* __restrict__ patch, const int (&tap)[4], const float (&w)[4],
                         float alpha, int c, float f) {
  if (alpha == 0.f) return f;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (tap[k] >= 0) q = fmaf(w[k], fminf(fmaxf(fmaf(t.gain, patch[tap[k] + c], t.off), 0.f), 1.f), q);
  return fmaf(1.f - alpha, f, q);
}

// RGB4: C == 3, Cp == 4 and enc 16-byte aligned (the image observation's case): the three channels in registers, the
// encoder input as one 16-byte store; the same arithmetic, so the same bits as the general loop
template <bool U8, bool RGB4>
__global__ void patch_apply_affine_k(const void* __restrict__ in, const float* __restrict__ patch,
                                     const float* __restrict__ tf, float* __restrict__ img, float* __restrict__ enc,
                                     long pixels, int H, int W, int C, int Cp, int ph, int pw, float shift) {
  const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= pixels) return;
  const int x = (int)(pix % W);
  const long r = pix / W;
  const int y = (int)(r % H);
  const PatchTf t = patch_tf_row(tf, r / H);
  int i0 = 0, j0 = 0;
  float fu = 0.f, fv = 0.f, alpha = 0.f, w[4] = {0.f, 0.f, 0.f, 0.f};
  int tap[4] = {-1, -1, -1, -1};  // element index of channel 0 of each in-range tap
  if (patch_coords(t, y, x, ph, pw, i0, j0, fu, fv)) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = i0 + (k >> 1), j = j0 + (k & 1);
      if (i >= 0 && i < ph && j >= 0 && j < pw) {
        w[k] = patch_tap_weight(k >> 1, k & 1, fu, fv);
        alpha += w[k];
        tap[k] = (i * pw + j) * C;
      }
    }
  }
  if constexpr (RGB4) {
    float f[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if constexpr (U8) f[c] = (float)static_cast<const uint8_t*>(in)[pix * 3 + c] / 255.0f;
      else f[c] = static_cast<const float*>(in)[pix * 3 + c];
      f[c] = patch_blend(t, patch, tap, w, alpha, c, f[c]);
    }
    if (img) {
#pragma unroll
      for (int c = 0; c < 3; ++c) img[pix * 3 + c] = f[c];
    }
    if (enc) reinterpret_cast<float4*>(enc)[pix] = make_float4(f[0] - shift, f[1] - shift, f[2] - shift, 0.f);
  } else {
    for (int c = 0; c < Cp; ++c) {
      float v = 0.f;
      if (c < C) {
        float f;
        if constexpr (U8) f = (float)static_cast<const uint8_t*>(in)[pix * C + c] / 255.0f;
        else f = static_cast<const float*>(in)[pix * C + c];
        f = patch_blend(t, patch, tap, w, alpha, c, f);
        if (img) img[pix * C + c] = f;
        v = f - shift;
      }
      if (enc) enc[pix * Cp + c] = v;
    }
  }
}

// part[k][e] = sum over the images n of chunk k (image order) of P'_n(patch[e]) * sum over the pixels (row-major) of
// w_n(pixel -> e) * d_image. The pixels come from the image-space bounding box of the patch-coordinate square
// (i - 1, i + 1) x (j - 1, j + 1), through the inverse of the row's 2 x 2 (padded against its rounding, clamped to
// the image; a non-finite inverse scans the whole image); every candidate's weight is re-formed as the forward does.
__global__ void patch_grad_affine_part_k(const float* __restrict__ dimg, const float* __restrict__ tf,
                                         const float* __restrict__ patch, float* __restrict__ part, int Nb, int H,
                                         int W, int C, int ph, int pw) {
  const int E = ph * pw * C;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int c = e % C, j = (e / C) % pw, i = e / (C * pw);
  const int n0 = blockIdx.y * SD_PATCH_CHUNK, n1 = min(Nb, n0 + SD_PATCH_CHUNK);
  const float p = patch ? patch[e] : 0.f;
  float s = 0.f;
  for (int n = n0; n < n1; ++n) {
    const PatchTf t = patch_tf_row(tf, n);
    const float rdet = 1.f / (t.a00 * t.a11 - t.a01 * t.a10);
    const float m00 = t.a11 * rdet, m01 = -t.a01 * rdet, m10 = -t.a10 * rdet, m11 = t.a00 * rdet;
    const float du = (float)i - t.b0, dv = (float)j - t.b1;
    const float yc = m00 * du + m01 * dv, xc = m10 * du + m11 * dv;
    const float hy = fabsf(m00) + fabsf(m01), hx = fabsf(m10) + fabsf(m11);
    const float py = 0.01f + 1e-5f * (fabsf(yc) + hy), px = 0.01f + 1e-5f * (fabsf(xc) + hx);
    // fmaxf / fminf return the other operand for a NaN: the bounds then span the image
    const int y_lo = (int)fminf(fmaxf(ceilf(yc - hy - py), 0.f), (float)H);
    const int y_hi = (int)fmaxf(fminf(floorf(yc + hy + py), (float)(H - 1)), -1.f);
    const int x_lo = (int)fminf(fmaxf(ceilf(xc - hx - px), 0.f), (float)W);
    const int x_hi = (int)fmaxf(fminf(floorf(xc + hx + px), (float)(W - 1)), -1.f);
    float a = 0.f;
    for (int y = y_lo; y <= y_hi; ++y)
      for (int x = x_lo; x <= x_hi; ++x) {
        int i0, j0;
        float fu, fv;
        if (!patch_coords(t, y, x, ph, pw, i0, j0, fu, fv)) continue;
        const int di = i - i0, dj = j - j0;
        if ((unsigned)di > 1u || (unsigned)dj > 1u) continue;
        a = fmaf(patch_tap_weight(di, dj, fu, fv), dimg[(((long)n * H + y) * W + x) * C + c], a);
      }
    const float q = fmaf(t.gain, p, t.off);
    s = fmaf((!patch || (q >= 0.f && q <= 1.f)) ? t.gain : 0.f, a, s);
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

extern "C" int sd_patch_apply_affine(const void* in, int in_u8, const float* patch, const float* tf, float* img,
                                     float* enc, int Nb, int H, int W, int C, int Cp, int ph, int pw, float shift,
                                     sd_stream stream_) {
  if (Nb <= 0) return SD_OK;
  if (!in || !patch || !tf || (!img && !enc) || H <= 0 || W <= 0 || C <= 0 || Cp < C || ph <= 0 || pw <= 0)
    return SD_EARG;
  const long pixels = (long)Nb * H * W;
  hipStream_t s = (hipStream_t)stream_;
  const bool rgb4 = C == 3 && Cp == 4 && ((uintptr_t)enc & 15) == 0;
  auto k = in_u8 ? (rgb4 ? patch_apply_affine_k<true, true> : patch_apply_affine_k<true, false>)
                 : (rgb4 ? patch_apply_affine_k<false, true> : patch_apply_affine_k<false, false>);
  k<<<sd_cdiv(pixels, 256), 256, 0, s>>>(in, patch, tf, img, enc, pixels, H, W, C, Cp, ph, pw, shift);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_patch_grad_affine(const float* dimg, const float* tf, float* dpatch, float* part, long part_floats,
                                    const float* patch, float w_tv, float* tv, int Nb, int H, int W, int C, int ph,
                                    int pw, sd_stream stream_) {
  if (!dimg || !tf || !dpatch || !part || Nb <= 0 || H <= 0 || W <= 0 || C <= 0 || ph <= 0 || pw <= 0)
    return SD_EARG;
  const int E = ph * pw * C, chunks = sd_cdiv(Nb, SD_PATCH_CHUNK);
  if (part_floats < (long)chunks * E || chunks > 65535) return SD_EARG;
  hipStream_t s = (hipStream_t)stream_;
  patch_grad_affine_part_k<<<dim3(sd_cdiv(E, 256), chunks), 256, 0, s>>>(dimg, tf, patch, part, Nb, H, W, C, ph, pw);
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
