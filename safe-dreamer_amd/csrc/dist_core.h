// Shared device math of the one-hot straight-through sampler (OneHotDist + F.gumbel_softmax(hard=True),
// distributions.py:16-33): used by the standalone sampler kernels (dist.hip) and by the fused RSSM scan (scan.hip).
#pragma once
#include "common.h"

namespace {

// ---------------------------------------------------------------- one-hot ST sampler
// Lanes [0, K) of a team of T lanes hold one categorical. Returns normalised unimix logits (nl) and p = softmax(l).
template <int T>
SD_DEV void unimix_forward(float l, bool act, int K, float unimix, float& p, float& pp, float& nl) {
  const float NEG = -INFINITY;
  float m = group_max<T>(act ? l : NEG);
  float e = act ? expf(l - m) : 0.f;
  float s = group_sum<T>(e);
  p = e / s;
  const float uni = unimix / (float)K;
  pp = p * (1.f - unimix) + uni;
  float lg = act ? logf(pp) : NEG;
  float m2 = group_max<T>(lg);
  float e2 = act ? expf(lg - m2) : 0.f;
  float s2 = group_sum<T>(e2);
  nl = act ? lg - (m2 + logf(s2)) : NEG;
}

// gradient of nl = log_softmax(log(p(1-u) + u/K)), p = softmax(l), w.r.t. l, given d_nl
template <int T>
SD_DEV float unimix_backward(float d_nl, float p, float pp, float nl, bool act, float unimix) {
  const float q = act ? expf(nl) : 0.f;  // softmax(lg)
  const float sd = group_sum<T>(act ? d_nl : 0.f);
  const float d_lg = d_nl - q * sd;
  const float d_p = act ? d_lg / pp * (1.f - unimix) : 0.f;
  const float sp = group_sum<T>(d_p * p);
  return act ? p * (d_p - sp) : 0.f;
}

// The smallest index among the team's lanes that hold its largest value (torch max(dim): the first maximum), on every
// lane. Inactive lanes pass a value below every active one and index 0x7fffffff.
template <int T>
SD_DEV int team_first_max(float best, int bi) {
#pragma unroll
  for (int o = T / 2; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  return bi;
}

template <int T>
SD_DEV void st_soft(float nl, float g, bool act, float& ys, int& idx, int lane_in_team) {
  const float y = act ? nl + g : -INFINITY;
  const float m = group_max<T>(y);
  const float e = act ? expf(y - m) : 0.f;
  const float s = group_sum<T>(e);
  ys = e / s;
  idx = team_first_max<T>(act ? ys : -1.f, act ? lane_in_team : 0x7fffffff);  // index of the largest soft value
}

// Straight-through gradient of a team's one-hot sample (sd_onehot_sample_bwd and the fused imagination backward): from
// the categorical's logit l (lane lt of the team, act = lt < K), its Gumbel noise gn and the upstream gradient d of the
// sample (0 on inactive lanes), d logit of <d, y_soft>. Everything is recomputed from the logits.
template <int T>
SD_DEV float st_sample_backward(float l, bool act, int K, float unimix, float gn, float d, int lt) {
  float p, pp, nl, ys;
  int idx;
  unimix_forward<T>(l, act, K, unimix, p, pp, nl);
  st_soft<T>(nl, gn, act, ys, idx, lt);
  const float sd = group_sum<T>(d * ys);
  return unimix_backward<T>(act ? ys * (d - sd) : 0.f, p, pp, nl, act, unimix);
}

// ---------------------------------------------------------------- bounded normal actor
// row r, action dim j of the head output x (rows, 2 A): loc = tanh(x[r, j]), sg = sigmoid(x[r, A + j] + 2) and
// scale() = (max_std - min_std) sg + min_std
struct BNormal {
  float loc, sg;
  SD_DEV float scale(float min_std, float max_std) const { return (max_std - min_std) * sg + min_std; }
};
SD_DEV BNormal bnormal_loc_scale(const float* x, long im, long is) {
  BNormal b;
  b.loc = tanhf(x[im]);
  b.sg = sigmoidf_(x[is] + 2.f);
  return b;
}
// Reparameterised gradient of the sampled, normalised action a / max(|a|, 1) (the divisor a constant, rssm.py:44):
// a = loc + eps sc, so d loc = d a and d sc = d a eps; d_mean / d_std are the gradients of x's [mean | std-logit].
SD_DEV void bnormal_sample_backward(const BNormal& b, float d_an, float action, float eps, float min_std, float max_std,
                                    float& d_mean, float& d_std) {
  const float da = d_an / fmaxf(fabsf(action), 1.f);
  d_mean = da * (1.f - b.loc * b.loc);
  d_std = da * eps * (max_std - min_std) * b.sg * (1.f - b.sg);
}

// ---------------------------------------------------------------- Deter GRU-style gates (rssm.py:65-75)
// backward of h' = u c + (1 - u) h, r = sigmoid(ra), c = tanh(r ca), u = sigmoid(ua - 1), given d = d h':
// the three gate gradients and d h
struct GruGrad {
  float dr, dc, du, dh;
};
SD_DEV GruGrad gru_gate_backward(float ra, float ca, float ua, float hv, float d) {
  const float rs = sigmoidf_(ra);
  const float c = tanhf(rs * ca);
  const float u = sigmoidf_(ua - 1.f);
  const float dtc = d * u * (1.f - c * c);
  GruGrad g;
  g.du = d * (c - hv) * u * (1.f - u);
  g.dc = dtc * rs;
  g.dr = dtc * ca * rs * (1.f - rs);
  g.dh = d * (1.f - u);
  return g;
}

}  // namespace
