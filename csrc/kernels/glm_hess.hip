// Newton statistics of generalised-linear-model posteriors: log-density, score and the negative
// Hessian of B parameter rows against N data rows in one pass over the data.
//
//   eta_bn = theta_b . x_n
//   logp_b = scale sum_n ll(y_n, eta_bn) + log prior(theta_b)
//   grad_b = scale sum_n r(y_n, eta_bn) x_n - prec theta_b
//   H_b    = scale sum_n w(eta_bn) x_n x_n^T + diag(prec)            (= -d^2 logp_b / d theta^2)
//
//   family      w
//   bernoulli   sigmoid(eta) (1 - sigmoid(eta))
//   poisson     exp(eta)
//   gaussian    inv_var
//
// ll, r, the prior and the constants that are left out are those of glm.hip; w comes from
// Link::eval_w of glm_elem.h, out of the same exponential and reciprocal. fp32, 1 <= D <= 64.
//
// The grid is (B, S): a workgroup of 256 threads owns one parameter row and the data tiles
// [s T / S, (s + 1) T / S) of split s. A tile of NF_GLM_TILE_N = 64 data rows is staged in LDS
// (glm::stage_tile: x_n zero-padded to the compile-time width DP, y_n beside it). Then
//   1. every thread takes part in eta: 4 adjacent lanes per data row, DP / 4 coordinates each
//      (theta in registers), completed with xor shuffles; lane 0 of a row evaluates the link
//      and writes w_n, r_n, ll_n to LDS (zeros for a padded row, which is not neutral for ll).
//      The dot product is summed in fp64 (its products are exact there) and rounded to fp32 once:
//      w = e^-|eta| / (1 + e^-|eta|)^2 has the relative error of eta's absolute error, and an
//      fp32 sum of terms of 1e3 that cancel to an eta of 5 would leave 1e-3 of it in w, which no
//      large sum of other rows hides in H as it does in log p and the score. The step is DP / 4
//      fp64 fma per thread and tile against 64 M (M + 1) fp32 ones in step 2;
//   2. after a barrier, the DP x DP accumulator is spread over registers as 16 x 16 micro-tiles
//      of M x M (M = DP / 16: 4 x 4 at DP = 64). Only the 136 micro-tiles on or above the
//      diagonal exist: threads 0 .. 135 own one each and do the rank-TN update
//      acc[j][k] = fmaf(w_n x_nj, x_nk, acc[j][k]) over the rows of the tile that exist. All
//      lanes of a wave read one LDS row at a time, 4 M-float segments of it at most 32 apart: a
//      broadcast read without bank conflicts. Threads 192 .. 192 + DP - 1 (a wave that owns no
//      micro-tile) sum the gradient column r_n x_nc meanwhile, thread 192 also ll_n.
// Each tile builds its partial from zero before it joins the running sum, so the error of a long
// sum grows with N / TN + TN. Split s writes its sums to work[s] ([S, B, D D + D + 1]: the D x D
// matrix of which only the entries j <= k are written and read, the gradient sums, the ll sum); a
// second kernel adds the partials in the order s = 0 .. S - 1, multiplies by scale, adds the
// prior terms and writes H[j][k] and H[k][j] from the one sum of (min, max), so H is symmetric
// bit for bit. No atomics anywhere: a result is bitwise repeatable for a given (B, N, D,
// n_splits), and a row's result depends neither on B nor on the row's place.
//
// The rank update is plain fmaf on the vector units; the f32-input MFMA was not tried.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no scratch anywhere):
//   DP   VGPRs (each of the three families)   LDS bytes   waves / SIMD
//   16   52                                   5120        8
//   32   64                                   9216        8
//   64   110                                  17408       4
// and 15 VGPRs, no LDS for the finalize kernel.
#include "glm_elem.h"
#include "glm_tiles.h"
#include "nf_common.h"

namespace nf {
namespace {

constexpr int TN = glm::TN;
constexpr int NT = 256;                    // threads of a workgroup
constexpr int LPR = 4;                     // lanes per data row in the eta step
constexpr int MG = 16;                     // micro-tiles per side of the accumulator
constexpr int NMT = MG * (MG + 1) / 2;     // micro-tiles on or above the diagonal
constexpr int GRAD0 = 192;                 // first thread of the gradient columns
using glm::FAM_BERNOULLI;
using glm::FAM_GAUSSIAN;
using glm::FAM_POISSON;
using glm::Link;

static_assert(TN * LPR == NT, "the eta step gives every data row of a tile LPR lanes");
static_assert(NMT <= GRAD0 && GRAD0 + 64 <= NT, "micro-tile and gradient threads are disjoint");

struct HessArgs {
  const float* theta;
  const float* X;
  const float* y;
  long ldt, ldx;   // row strides in elements (unit inner stride)
  float inv_var;   // gaussian family only
  float* work;     // [S, B, D D + D + 1]
  int B, N, D, S;
};

// glm::part_sum<LPR> for the fp64 sum of eta: every lane of a row gets the same bits
__device__ __forceinline__ double lane_sum(double v) {
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int DP, int FAMILY>
__global__ __launch_bounds__(NT) void glm_hess_kernel(HessArgs a) {
  constexpr int C = DP / LPR, M = DP / MG;
  __shared__ __align__(16) float tx[TN * DP];
  __shared__ float ty[TN], tw[TN], tr[TN], tl[TN];
  const int tid = threadIdx.x;
  const long b = blockIdx.x;
  const int split = blockIdx.y;
  const Link<FAMILY> link(a.inv_var);

  // eta step: data row erow of the tile, coordinates [part C, (part + 1) C)
  const int part = tid % LPR, erow = tid / LPR;
  float th[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int gc = part * C + c;
    th[c] = gc < a.D ? a.theta[b * a.ldt + gc] : 0.f;
  }

  // micro-tile (mj, mk), mj <= mk, of thread tid < NMT: row mj holds MG - mj of them
  const bool hess = tid < NMT;
  int mj = 0, mk = 0;
  if (hess) {
    int rem = tid;
    while (rem >= MG - mj) {
      rem -= MG - mj;
      ++mj;
    }
    mk = mj + rem;
  }
  const int gcol = tid - GRAD0;   // gradient column of threads GRAD0 .. GRAD0 + DP - 1
  const bool gradt = gcol >= 0 && gcol < DP;

  float acc[M][M], gacc = 0.f, lacc = 0.f;
#pragma unroll
  for (int j = 0; j < M; ++j)
#pragma unroll
    for (int k = 0; k < M; ++k) acc[j][k] = 0.f;

  const long nt = ((long)a.N + TN - 1) / TN;
  const long t0 = split * nt / a.S, t1 = (split + 1) * nt / a.S;
  for (long t = t0; t < t1; ++t) {
    const long n0 = t * TN;
    const int nn = (int)(a.N - n0 < TN ? a.N - n0 : TN);
    __syncthreads();
    glm::stage_tile<DP, NT>(a.X, a.ldx, a.y, a.N, a.D, n0, tx, ty);
    __syncthreads();
    {
      const float* xn = tx + erow * DP + part * C;
      double eta = 0.0;
#pragma unroll
      for (int c = 0; c < C; ++c) eta = fma((double)th[c], (double)xn[c], eta);
      eta = lane_sum(eta);
      if (part == 0) {
        float ll = 0.f, r = 0.f, w = 0.f;
        if (erow < nn) link.eval_w(ty[erow], (float)eta, ll, r, w);
        tw[erow] = w;
        tr[erow] = r;
        tl[erow] = ll;
      }
    }
    __syncthreads();
    if (hess) {
      float ht[M][M];
#pragma unroll
      for (int j = 0; j < M; ++j)
#pragma unroll
        for (int k = 0; k < M; ++k) ht[j][k] = 0.f;
      const float* xj = tx + mj * M;
      const float* xk = tx + mk * M;
#pragma unroll 4   // four rows of LDS reads in flight: a workgroup has one wave per SIMD
      for (int n = 0; n < nn; ++n) {
        const float w = tw[n];
        float vk[M];
#pragma unroll
        for (int k = 0; k < M; ++k) vk[k] = xk[n * DP + k];
#pragma unroll
        for (int j = 0; j < M; ++j) {
          const float wj = w * xj[n * DP + j];
#pragma unroll
          for (int k = 0; k < M; ++k) ht[j][k] = fmaf(wj, vk[k], ht[j][k]);
        }
      }
#pragma unroll
      for (int j = 0; j < M; ++j)
#pragma unroll
        for (int k = 0; k < M; ++k) acc[j][k] += ht[j][k];
    } else if (gradt) {
      float gt = 0.f;
      for (int n = 0; n < nn; ++n) gt = fmaf(tr[n], tx[n * DP + gcol], gt);
      gacc += gt;
      if (gcol == 0) {
        float lt = 0.f;
        for (int n = 0; n < nn; ++n) lt += tl[n];
        lacc += lt;
      }
    }
  }

  const long E = (long)a.D * a.D + a.D + 1;
  float* out = a.work + ((long)split * a.B + b) * E;
  if (hess) {
#pragma unroll
    for (int j = 0; j < M; ++j)
#pragma unroll
      for (int k = 0; k < M; ++k) {
        const int gj = mj * M + j, gk = mk * M + k;
        if (gj <= gk && gk < a.D) out[(long)gj * a.D + gk] = acc[j][k];
      }
  } else if (gradt) {
    if (gcol < a.D) out[(long)a.D * a.D + gcol] = gacc;
    if (gcol == 0) out[(long)a.D * a.D + a.D] = lacc;
  }
}

struct HessFinalArgs {
  const float* work;
  const float* theta;
  long ldt;
  const float* prec_dev;   // [D], or null -> prec_host
  float prec_host, scale;
  int has_prior;
  float* logp;   // [B]
  float* grad;   // [B, D]
  float* hess;   // [B, D, D]
  int B, D, S;
};

// a summed entry (j, k) of the matrix -> H: times scale, plus prec_j on the diagonal
__device__ __forceinline__ float finish_hess(float sum, float scale, const glm::Prior& pr, int j,
                                             int k) {
#pragma clang fp contract(off)   // the product is rounded on its own, as written
  sum *= scale;
  if (pr.has_prior && j == k) sum += pr.prec(j);
  return sum;
}

// One thread per element e of [B, D D + D + 1]: the partials of e in the order s = 0 .. S - 1
// (of (min(j, k), max(j, k)) for a matrix entry: the lower triangle mirrors the upper), times
// scale, plus the prior's term; gradient columns and log p as glm_finalize_kernel has them.
__global__ __launch_bounds__(256) void glm_hess_finalize_kernel(HessFinalArgs a) {
  const long DD = (long)a.D * a.D, E = DD + a.D + 1;
  const long n = (long)a.B * E;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const long i = e / E, c = e % E;
  long src = c;
  int j = 0, k = 0;
  if (c < DD) {
    j = (int)(c / a.D), k = (int)(c % a.D);
    src = j <= k ? c : (long)k * a.D + j;
  }
  float sum = 0.f;
  for (int s = 0; s < a.S; ++s) sum += a.work[((long)s * a.B + i) * E + src];
  const glm::Prior pr{a.prec_dev, a.prec_host, a.has_prior};
  const float* th = a.theta + i * a.ldt;
  if (c < DD) {
    a.hess[i * DD + c] = finish_hess(sum, a.scale, pr, j, k);
  } else if (c < DD + a.D) {
    const int d = (int)(c - DD);
    a.grad[i * a.D + d] = glm::finish_grad(sum, a.scale, pr, d, th[d]);
  } else {
    float q = 0.f, cst = 0.f;
    if (a.has_prior) {
      for (int d = 0; d < a.D; ++d) q = glm::prior_quad(q, pr.prec(d), th[d]);
      cst = glm::log_prior_const(pr, a.D);
    }
    a.logp[i] = glm::finish_logp(sum, a.scale, pr, q, cst);
  }
}

template <int DP>
void launch_hess(const HessArgs& a, int family, hipStream_t stream) {
  const dim3 grid((unsigned)a.B, (unsigned)a.S), block(NT);
  if (family == FAM_BERNOULLI)
    hipLaunchKernelGGL((glm_hess_kernel<DP, FAM_BERNOULLI>), grid, block, 0, stream, a);
  else if (family == FAM_POISSON)
    hipLaunchKernelGGL((glm_hess_kernel<DP, FAM_POISSON>), grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL((glm_hess_kernel<DP, FAM_GAUSSIAN>), grid, block, 0, stream, a);
  NF_HIP_CHECK(hipGetLastError());
}

}  // namespace
}  // namespace nf

using namespace nf;

int nf_glm_hess_splits(int B, int N, int D, int n_splits) {
  (void)D;
  const long nt = ((long)N + TN - 1) / TN;
  long S = n_splits;
  // a workgroup per (row, split): 2048 of them, two rounds of the four that fit a CU, while B
  // allows it, at most 512 splits (the finalize kernel adds them one after the other); never more
  // splits than data tiles
  if (S <= 0) {
    S = (2048 + (long)B - 1) / (B > 0 ? B : 1);
    if (S > 512) S = 512;
  }
  if (S > nt) S = nt;
  return S < 1 ? 1 : (int)S;
}

void nf_launch_glm_logp_grad_hess(const float* theta, long ldt, const float* X, long ldx,
                                  const float* y, const float* prec_dev, float prec_host,
                                  int has_prior, int family, float inv_var, float scale, int S,
                                  float* logp, float* grad, float* hess, float* work, int B, int N,
                                  int D, hipStream_t stream) {
  if (B <= 0 || N <= 0) return;
  const HessArgs a{theta, X, y, ldt, ldx, inv_var, work, B, N, D, S};
  if (D <= 16) launch_hess<16>(a, family, stream);
  else if (D <= 32) launch_hess<32>(a, family, stream);
  else launch_hess<64>(a, family, stream);

  const HessFinalArgs f{work, theta, ldt, prec_dev, prec_host, scale, has_prior, logp, grad, hess,
                        B, D, S};
  const long n = (long)B * ((long)D * D + D + 1);
  hipLaunchKernelGGL(glm_hess_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     stream, f);
  NF_HIP_CHECK(hipGetLastError());
}
