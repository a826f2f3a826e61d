// Generalised-linear-model posteriors: log-density and score of B parameter rows against N data
// rows in one pass.
//
//   eta_in = theta_i . x_n
//   logp_i = scale sum_n ll(y_n, eta_in) + log prior(theta_i)
//   grad_i = scale sum_n r(y_n, eta_in) x_n - prec theta_i
//
//   family      ll                          r
//   bernoulli   y eta - softplus(eta)       y - sigmoid(eta)
//   poisson     y eta - exp(eta)            y - exp(eta)
//   gaussian    -0.5 inv_var (y - eta)^2    inv_var (y - eta)
//
// fp32, 1 <= D <= 64; the [B, N] matrix of eta is never stored. The terms of ll that do not
// depend on theta (-lgamma(y + 1), -0.5 N log(2 pi / inv_var)) are not summed here: the caller
// adds them once. log prior = -0.5 sum prec_c theta_c^2 + 0.5 sum log prec_c - D/2 log 2 pi over
// the coordinates with prec_c > 0; a coordinate with prec_c = 0 is flat and adds nothing.
//
// A workgroup owns NF_GLM_TILE_B rows i of theta. Row i lives in registers (theta_i, the
// gradient accumulator and the gradient partial of the current tile), split over LPR adjacent
// lanes of C coordinates each for D > 16 (C = 16, LPR = 2 or 4, the instantiations of stein.hip);
// eta is then completed with LPR-wide xor shuffles. Tiles of NF_GLM_TILE_N data rows are staged
// in LDS as x_n zero-padded to the compile-time width C LPR, with y_n beside them; every lane of
// a part reads the same n, a broadcast read. Each tile is summed into a partial of its own before
// it joins the running sum, so the error of a long sum grows with N / TILE_N + TILE_N, not N.
// The row loop of a tile runs over the rows that exist (a padded row is not neutral: ll(0, 0) is
// -log 2 for the Bernoulli link); its trip count depends on N alone, nothing exits on data.
//
// The grid is (b-tiles, n_splits): split s takes the data tiles [s T / S, (s + 1) T / S) and
// writes its partial sums to work[s] ([S, B, D + 1]: D gradient sums, then the ll sum); a second
// kernel adds the partials in the order s = 0 .. S - 1, multiplies by scale and adds the prior
// terms. No atomics anywhere, so a result is bitwise repeatable for a given (B, N, D, n_splits),
// and a row's result depends neither on B nor on the row's place in its tile.
//
// Transcendentals: the hardware forms v_exp_f32 / v_log_f32 / v_rcp_f32 (1 ulp each). The
// Bernoulli link takes softplus and sigmoid from one e = exp(-|eta|) in (0, 1], so the log sees
// an argument in (1, 2] and nothing overflows at any eta; ll is summed as (y eta - max(eta, 0)) -
// log(1 + e), which keeps the small term when y eta and max(eta, 0) cancel. The exponent's
// argument error (|eta| 2^-24 relative) is far inside the 1e-4 abs-sum limit of
// tests/test_glm_gpu.py, which is what decided for the hardware forms over expf / log1pf. The
// Poisson link overflows as IEEE does (exp(eta) = inf beyond eta ~ 88.7).
#include "glm_elem.h"
#include "glm_tiles.h"
#include "nf_common.h"

namespace nf {
namespace {

constexpr int TB = NF_GLM_TILE_B;
constexpr int TN = glm::TN;
using glm::FAM_BERNOULLI;
using glm::FAM_GAUSSIAN;
using glm::FAM_POISSON;
using glm::Link;

struct GlmArgs {
  const float* theta;
  const float* X;
  const float* y;
  long ldt, ldx;   // row strides in elements (unit inner stride)
  float inv_var;   // gaussian family only
  float* work;     // [S, B, D + 1]
  int B, N, D, S;
};

// The links, the lane sum, the tile staging and the row loop of a tile: glm_elem.h, shared with
// the trajectory kernel of glm_hmc.hip.
template <int C, int LPR, int FAMILY>
__global__ __launch_bounds__(TB* LPR) void glm_pairs_kernel(GlmArgs a) {
  constexpr int DP = C * LPR, NT = TB * LPR;
  __shared__ __align__(16) float tx[TN * DP];
  __shared__ float ty[TN];
  const int part = threadIdx.x % LPR, row = threadIdx.x / LPR;
  const long i = (long)blockIdx.x * TB + row;
  const int split = blockIdx.y;
  const Link<FAMILY> link(a.inv_var);

  float th[C], acc[C], lacc = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int gc = part * C + c;
    th[c] = (i < a.B && gc < a.D) ? a.theta[i * a.ldt + gc] : 0.f;
    acc[c] = 0.f;
  }

  const long nt = ((long)a.N + TN - 1) / TN;
  const long t0 = split * nt / a.S, t1 = (split + 1) * nt / a.S;
  for (long t = t0; t < t1; ++t) {
    const long n0 = t * TN;
    const int nn = (int)(a.N - n0 < TN ? a.N - n0 : TN);
    __syncthreads();
    glm::stage_tile<DP, NT>(a.X, a.ldx, a.y, a.N, a.D, n0, tx, ty);
    __syncthreads();
    glm::tile_rows<C, LPR, FAMILY>(link, th, tx, ty, part, nn, acc, lacc);
  }

  if (i < a.B) {
    float* out = a.work + ((long)split * a.B + i) * (a.D + 1);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int gc = part * C + c;
      if (gc < a.D) out[gc] = acc[c];
    }
    if (part == 0) out[a.D] = lacc;
  }
}

struct GlmFinalArgs {
  const float* work;
  const float* theta;
  long ldt;
  const float* prec_dev;   // [D], or null -> prec_host
  float prec_host, scale;
  int has_prior;
  float* logp;   // [B]
  float* grad;   // [B, D]
  int B, D, S;
};

// One thread per element e of [B, D + 1]: the partials of e in the order s = 0 .. S - 1, times
// scale, plus the prior's term (-prec_c theta_ic for a gradient column, log prior_i for c = D).
__global__ __launch_bounds__(256) void glm_finalize_kernel(GlmFinalArgs a) {
  const long n = (long)a.B * (a.D + 1);
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const long i = e / (a.D + 1);
  const int c = (int)(e % (a.D + 1));
  float sum = 0.f;
  for (int s = 0; s < a.S; ++s) sum += a.work[(long)s * n + e];
  const glm::Prior pr{a.prec_dev, a.prec_host, a.has_prior};
  const float* th = a.theta + i * a.ldt;
  if (c < a.D) {
    a.grad[i * a.D + c] = glm::finish_grad(sum, a.scale, pr, c, th[c]);
  } else {
    float q = 0.f, cst = 0.f;
    if (a.has_prior) {
      for (int d = 0; d < a.D; ++d) q = glm::prior_quad(q, pr.prec(d), th[d]);
      cst = glm::log_prior_const(pr, a.D);
    }
    a.logp[i] = glm::finish_logp(sum, a.scale, pr, q, cst);
  }
}

template <int C, int LPR>
void launch_pairs(const GlmArgs& a, int family, hipStream_t stream) {
  const dim3 grid((unsigned)(((long)a.B + TB - 1) / TB), (unsigned)a.S), block(TB * LPR);
  if (family == FAM_BERNOULLI)
    hipLaunchKernelGGL((glm_pairs_kernel<C, LPR, FAM_BERNOULLI>), grid, block, 0, stream, a);
  else if (family == FAM_POISSON)
    hipLaunchKernelGGL((glm_pairs_kernel<C, LPR, FAM_POISSON>), grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL((glm_pairs_kernel<C, LPR, FAM_GAUSSIAN>), grid, block, 0, stream, a);
  NF_HIP_CHECK(hipGetLastError());
}

}  // namespace
}  // namespace nf

using namespace nf;

int nf_glm_splits(int B, int N, int D, int n_splits) {
  (void)D;
  const long bt = ((long)B + TB - 1) / TB, nt = ((long)N + TN - 1) / TN;
  long S = n_splits;
  // enough workgroups for the whole card at small B; never more splits than data tiles
  if (S <= 0) {
    S = (1024 + bt - 1) / (bt > 0 ? bt : 1);
    if (S > 64) S = 64;
  }
  if (S > nt) S = nt;
  return S < 1 ? 1 : (int)S;
}

void nf_launch_glm_logp_grad(const float* theta, long ldt, const float* X, long ldx,
                             const float* y, const float* prec_dev, float prec_host,
                             int has_prior, int family, float inv_var, float scale, int S,
                             float* logp, float* grad, float* work, int B, int N, int D,
                             hipStream_t stream) {
  if (B <= 0 || N <= 0) return;
  const GlmArgs a{theta, X, y, ldt, ldx, inv_var, work, B, N, D, S};
  if (D <= 1) launch_pairs<1, 1>(a, family, stream);
  else if (D <= 2) launch_pairs<2, 1>(a, family, stream);
  else if (D <= 4) launch_pairs<4, 1>(a, family, stream);
  else if (D <= 8) launch_pairs<8, 1>(a, family, stream);
  else if (D <= 16) launch_pairs<16, 1>(a, family, stream);
  else if (D <= 32) launch_pairs<16, 2>(a, family, stream);
  else launch_pairs<16, 4>(a, family, stream);

  const GlmFinalArgs f{work, theta, ldt, prec_dev, prec_host, scale, has_prior, logp, grad,
                       B, D, S};
  const long n = (long)B * (D + 1);
  hipLaunchKernelGGL(glm_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     f);
  NF_HIP_CHECK(hipGetLastError());
}
