// Device-side pieces shared by the GLM kernels (glm.hip: one log-density / score pass;
// glm_hmc.hip: a whole leapfrog trajectory of such passes; glm_hess.hip: a pass with curvature): the links of the three families, the
// sum over the lanes that share a parameter row, the staging of a data tile in LDS, the row loop
// of one tile and the prior / scale step that turns the summed partials into log p and the score.
// Both kernels go through the same functions, so a pass inside a trajectory has the bits of the
// stand-alone pass (tests/test_hmc_gpu.py pins that).
#pragma once

#include <hip/hip_runtime.h>

#include "glm_tiles.h"

namespace nf {
namespace glm {

constexpr int TN = NF_GLM_TILE_N;
constexpr int FAM_BERNOULLI = 0, FAM_POISSON = 1, FAM_GAUSSIAN = 2;
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
constexpr float HALF_LOG_2PI = 0.9189385332046727f;

// ll and r of one (y, eta) pair; eval_w adds the weight w = -d r / d eta of the Hessian
// (glm_hess.hip)
template <int FAMILY>
struct Link;

template <>
struct Link<FAM_BERNOULLI> {
  __device__ explicit Link(float) {}
  __device__ __forceinline__ void eval(float y, float eta, float& ll, float& r) const {
    const float e = __builtin_amdgcn_exp2f(-fabsf(eta) * LOG2E);   // e^(-|eta|)
    const float inv = __builtin_amdgcn_rcpf(1.f + e);
    const float l1p = __builtin_amdgcn_logf(1.f + e) * LN2;        // log1p(e), 1 + e in (1, 2]
    ll = fmaf(y, eta, -fmaxf(eta, 0.f)) - l1p;
    r = y - (eta >= 0.f ? inv : e * inv);
  }
  // eval and the weight w = sigmoid(eta) (1 - sigmoid(eta)) = e / (1 + e)^2 from the same e and
  // inv: it underflows to 0 at large |eta|, nothing overflows
  __device__ __forceinline__ void eval_w(float y, float eta, float& ll, float& r, float& w) const {
    const float e = __builtin_amdgcn_exp2f(-fabsf(eta) * LOG2E);
    const float inv = __builtin_amdgcn_rcpf(1.f + e);
    const float l1p = __builtin_amdgcn_logf(1.f + e) * LN2;
    ll = fmaf(y, eta, -fmaxf(eta, 0.f)) - l1p;
    r = y - (eta >= 0.f ? inv : e * inv);
    w = e * inv * inv;
  }
};

template <>
struct Link<FAM_POISSON> {
  __device__ explicit Link(float) {}
  __device__ __forceinline__ void eval(float y, float eta, float& ll, float& r) const {
    const float ex = __builtin_amdgcn_exp2f(eta * LOG2E);
    ll = fmaf(y, eta, -ex);
    r = y - ex;
  }
  // eval and the weight w = exp(eta) (IEEE overflow, as r)
  __device__ __forceinline__ void eval_w(float y, float eta, float& ll, float& r, float& w) const {
    const float ex = __builtin_amdgcn_exp2f(eta * LOG2E);
    ll = fmaf(y, eta, -ex);
    r = y - ex;
    w = ex;
  }
};

template <>
struct Link<FAM_GAUSSIAN> {
  float inv_var;
  __device__ explicit Link(float iv) : inv_var(iv) {}
  __device__ __forceinline__ void eval(float y, float eta, float& ll, float& r) const {
    const float d = y - eta;
    r = inv_var * d;
    ll = (-0.5f * r) * d;
  }
  // eval and the constant weight w = inv_var
  __device__ __forceinline__ void eval_w(float y, float eta, float& ll, float& r, float& w) const {
    eval(y, eta, ll, r);
    w = inv_var;
  }
};

// sum over the LPR adjacent lanes that share a row; every one of them gets the same bits
template <int LPR>
__device__ __forceinline__ float part_sum(float v) {
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// rows [n0, n0 + TN) of X [N, D] (row stride ldx) and y -> tx[n][DP], ty[n]; zero beyond N and
// beyond D. NT threads take part.
template <int DP, int NT>
__device__ __forceinline__ void stage_tile(const float* X, long ldx, const float* y, int N, int D,
                                           long n0, float* tx, float* ty) {
  for (int idx = threadIdx.x; idx < TN * DP; idx += NT) {
    const int n = idx / DP, c = idx % DP;
    const long gn = n0 + n;
    tx[idx] = (gn < N && c < D) ? X[gn * ldx + c] : 0.f;
  }
  for (int n = threadIdx.x; n < TN; n += NT) ty[n] = (n0 + n < N) ? y[n0 + n] : 0.f;
}

// The nn existing rows of the staged tile against the C coordinates th of this lane's part of a
// parameter row: the tile's partial sums (gradient gt, log-likelihood lt) are built from zero and
// then join the running sums acc and lacc.
template <int C, int LPR, int FAMILY>
__device__ __forceinline__ void tile_rows(const Link<FAMILY>& link, const float (&th)[C],
                                          const float* tx, const float* ty, int part, int nn,
                                          float (&acc)[C], float& lacc) {
  constexpr int DP = C * LPR;
  float gt[C], lt = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) gt[c] = 0.f;
  const auto add_row = [&](int n) {
    const float* xn = tx + n * DP + part * C;
    float eta = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) eta = fmaf(th[c], xn[c], eta);
    eta = part_sum<LPR>(eta);
    float ll, r;
    link.eval(ty[n], eta, ll, r);
    lt += ll;
#pragma unroll
    for (int c = 0; c < C; ++c) gt[c] = fmaf(r, xn[c], gt[c]);
  };
  // one row per trip: two rows by hand raised the D > 32 instantiations from 94 to 156 VGPRs
  // and measured 1.45x slower there, no faster elsewhere (docs/PERF_NOTES.md)
  for (int n = 0; n < nn; ++n) add_row(n);
  lacc += lt;
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] += gt[c];
}

// The prior of a pass. prec_dev [D] when not null, else prec_host.
struct Prior {
  const float* prec_dev;
  float prec_host;
  int has_prior;
  __device__ __forceinline__ float prec(int c) const { return prec_dev ? prec_dev[c] : prec_host; }
};

// a summed gradient column -> the score: times scale, minus prec_c theta_c
__device__ __forceinline__ float finish_grad(float sum, float scale, const Prior& pr, int c,
                                             float theta_c) {
#pragma clang fp contract(off)   // the product is rounded on its own, as written
  sum *= scale;
  if (pr.has_prior) sum = fmaf(-pr.prec(c), theta_c, sum);
  return sum;
}

// the theta-free part of the log prior: 0.5 sum log prec_c - k / 2 log 2 pi over the k
// coordinates with prec_c > 0
__device__ __forceinline__ float log_prior_const(const Prior& pr, int D) {
  float lg = 0.f;
  int k = 0;
  for (int d = 0; d < D; ++d) {
    const float p = pr.prec(d);
    if (p > 0.f) {
      lg += logf(p);
      ++k;
    }
  }
  return fmaf(0.5f, lg, -HALF_LOG_2PI * (float)k);
}

// one more coordinate of q = sum_d prec_d theta_d^2 (ascending d)
__device__ __forceinline__ float prior_quad(float q, float prec_d, float theta_d) {
  return fmaf(prec_d * theta_d, theta_d, q);
}

// the summed log-likelihood -> log p: times scale, plus the log prior built from q and the
// constant of log_prior_const
__device__ __forceinline__ float finish_logp(float sum, float scale, const Prior& pr, float q,
                                             float cst) {
#pragma clang fp contract(off)   // the product is rounded before the prior joins it
  sum *= scale;
  if (pr.has_prior) sum += fmaf(-0.5f, q, cst);
  return sum;
}

}  // namespace glm
}  // namespace nf
