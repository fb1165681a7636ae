// What the ConvEncoder stage kernels share: the norm-weight argument of the fused conv epilogues (conv.hip) and of the
// pool / RMSNorm row kernels (poolnorm.hip).
#pragma once
#include "common.h"

namespace {
// FiLM stage (multimodal encoder): y = silu(gamma[n / ipc][c] * norm + beta[n / ipc][c]) with gamma / beta (rows, C)
// f32 and ipc images per context row. The stage kernels take their norm weight as a type NW: `const float*` is the
// plain stage (signature and code as before), FilmNW adds the modulation. A tile can span images of two context rows
// (8 x 8 stage: two images per 128 pixels), so gamma / beta are read per pooled pixel, not once per workgroup.
struct FilmNW {
  const float* nw;
  const float* gamma;
  const float* beta;
  int ipc;
};
template <class NW> constexpr bool is_film = false;
template <> constexpr bool is_film<FilmNW> = true;
SD_DEV const float* nw_of(const float* nw) { return nw; }
SD_DEV const float* nw_of(const FilmNW& f) { return f.nw; }
}  // namespace
