// Hamiltonian Monte Carlo on generalised-linear-model posteriors: a whole trajectory of L leapfrog
// steps and the Metropolis accept step of B chains in one launch.
//
//   h = eps_i / 2, and L times
//     p     = fma(h, g, p)                  half kick
//     theta = fma(eps_i minv_c, p, theta)   drift (minv_c = 1 without a mass)
//     (lp, g) = log p and score at theta    one pass over the N data rows, as in glm.hip
//     p     = fma(h, g, p)                  half kick
//   kin(p) = 0.5 sum_c minv_c p_c^2
//   dH     = (kin(p_L) - kin(p_0)) + (logp_0 - lp_L)
//   accept = isfinite(dH) && log_u_i < -dH
//
// The two half kicks of consecutive steps are not merged (one fma per coordinate per step against
// an N D pass), so L steps in one launch are bitwise L launches of one step. log p is the
// const-free one of glm.hip; the constant cancels in dH.
//
// The layout is that of glm_pairs_kernel: a workgroup owns R chains; a chain's theta, its running
// gradient and the gradient partial of the current tile live in registers, split over LPR adjacent
// lanes of C coordinates each for D > 16; tiles of NF_GLM_TILE_N data rows are staged zero-padded
// in LDS and read as broadcasts. A trajectory is sequential and a grid has no barrier, so there is
// no split over N: every workgroup walks all data tiles in order, L times, and the prior and scale
// are applied in the kernel with the operations of glm_finalize_kernel at S = 1 (glm_elem.h holds
// the code both kernels run). (lp_L, g_L) are therefore bitwise what glm_logp_grad(theta_prop,
// n_splits = 1) returns, and a chain's result depends only on the order of the data tiles: not on
// R, not on its place in the tile, not on B.
//
// The momentum is not needed during a data pass. With PARK it waits in the chain's row of p_prop
// (written after the drift, read back before the second kick, by the same lane), which keeps the
// momentum out of the registers of the pass (13 - 14 VGPRs at the widths of 16); without PARK it
// stays in registers. docs/PERF_NOTES.md ("HMC trajectory") has the register counts and the
// measurement that chose.
//
// R is 128, 64 or 32 (a workgroup has at least 64 threads; at R = 32 and D <= 16 the upper half
// of the lanes only helps staging). The grid is ceil(B / R) workgroups, so a small R is what fills
// the card at sampler-sized B. Trip counts are fixed by L and N: nothing exits or loops on data, a
// diverged chain (inf or nan theta) runs to the end and is rejected. No atomics.
#include "glm_elem.h"
#include "nf_common.h"

#ifndef NF_HMC_PARK
#define NF_HMC_PARK 1
#endif

namespace nf {
namespace {

using glm::TN;

struct HmcArgs {
  const float* theta0;   // [B, D], row stride ldt
  const float* p0;       // [B, D]
  const float* logp0;    // [B]
  const float* grad0;    // [B, D]
  const float* eps;      // [B]
  const float* minv;     // [D] or null
  const float* log_u;    // [B]
  const float* X;        // [N, D], row stride ldx
  const float* y;        // [N]
  long ldt, ldx;
  glm::Prior prior;
  float inv_var, scale;
  float* theta_prop;     // [B, D]
  float* p_prop;         // [B, D]
  float* theta_out;      // [B, D]
  float* logp_out;       // [B]
  float* grad_out;       // [B, D]
  float* accept;         // [B]
  float* dH;             // [B]
  int B, N, D, L;
};

constexpr int hmc_threads(int R, int LPR) { return R * LPR < 64 ? 64 : R * LPR; }

template <int C, int LPR, int FAMILY, int R>
__global__ __launch_bounds__(hmc_threads(R, LPR)) void glm_hmc_kernel(HmcArgs a) {
  constexpr int DP = C * LPR, NT = hmc_threads(R, LPR);
  __shared__ __align__(16) float tx[TN * DP];
  __shared__ float ty[TN];
  const int part = threadIdx.x % LPR, row = threadIdx.x / LPR;
  const long i = (long)blockIdx.x * R + row;
  const bool live = row < R && i < a.B;   // a dead lane stages tiles and computes on zeros
  const glm::Link<FAMILY> link(a.inv_var);
  const glm::Prior pr = a.prior;
  const int lane0 = (int)(threadIdx.x % 64) - part;   // first lane of this chain's parts
  // this lane's coordinates that exist: c < nc (none in a dead lane)
  const int left = a.D - part * C;
  const int nc = live ? (left < 0 ? 0 : (left > C ? C : left)) : 0;

  const float eps = live ? a.eps[i] : 0.f;
  const float h = 0.5f * eps;
  const float cst = pr.has_prior ? glm::log_prior_const(pr, a.D) : 0.f;

  float th[C], g[C], p[C];
  float kin0 = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int gc = part * C + c;
    const bool on = c < nc;
    th[c] = on ? a.theta0[i * a.ldt + gc] : 0.f;
    g[c] = on ? a.grad0[i * a.D + gc] : 0.f;
    p[c] = on ? a.p0[i * a.D + gc] : 0.f;
    const float mi = (on && a.minv) ? a.minv[gc] : 1.f;
    kin0 = fmaf(mi * p[c], p[c], kin0);
  }
  kin0 = 0.5f * glm::part_sum<LPR>(kin0);

  const long nt = ((long)a.N + TN - 1) / TN;
  float lp = 0.f;
  for (int step = 0; step < a.L; ++step) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int gc = part * C + c;
      const bool on = c < nc;
      const float mi = (on && a.minv) ? a.minv[gc] : 1.f;
      if (on) {
        p[c] = fmaf(h, g[c], p[c]);
        th[c] = fmaf(eps * mi, p[c], th[c]);
#if NF_HMC_PARK
        a.p_prop[i * a.D + gc] = p[c];
#endif
      }
      g[c] = 0.f;
    }

    float lacc = 0.f;
    for (long t = 0; t < nt; ++t) {
      const long n0 = t * TN;
      const int nn = (int)(a.N - n0 < TN ? a.N - n0 : TN);
      __syncthreads();
      glm::stage_tile<DP, NT>(a.X, a.ldx, a.y, a.N, a.D, n0, tx, ty);
      __syncthreads();
      glm::tile_rows<C, LPR, FAMILY>(link, th, tx, ty, part, nn, g, lacc);
    }

    // the prior's quadratic form in ascending coordinate order: the parts take turns
    float q = 0.f;
    if (pr.has_prior) {
#pragma unroll
      for (int pp = 0; pp < LPR; ++pp) {
        float qq = q;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int gc = pp * C + c;
          if (gc < a.D) qq = glm::prior_quad(qq, pr.prec(gc), th[c]);
        }
        q = LPR > 1 ? __shfl(qq, lane0 + pp, 64) : qq;
      }
    }
    lp = glm::finish_logp(0.f + lacc, a.scale, pr, q, cst);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int gc = part * C + c;
      if (c < nc) {
        g[c] = glm::finish_grad(0.f + g[c], a.scale, pr, gc, th[c]);
#if NF_HMC_PARK
        p[c] = a.p_prop[i * a.D + gc];
#endif
        p[c] = fmaf(h, g[c], p[c]);
      } else {
        g[c] = 0.f;
      }
    }
  }

  float kin1 = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int gc = part * C + c;
    const float mi = (c < nc && a.minv) ? a.minv[gc] : 1.f;
    kin1 = fmaf(mi * p[c], p[c], kin1);
  }
  kin1 = 0.5f * glm::part_sum<LPR>(kin1);

  if (!live) return;
  const float lp0 = a.logp0[i];
  const float dH = (kin1 - kin0) + (lp0 - lp);
  const bool acc = isfinite(dH) && a.log_u[i] < -dH;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int gc = part * C + c;
    if (c < nc) {
      const long o = i * a.D + gc;
      a.theta_prop[o] = th[c];
      a.p_prop[o] = p[c];
      a.theta_out[o] = acc ? th[c] : a.theta0[i * a.ldt + gc];
      a.grad_out[o] = acc ? g[c] : a.grad0[o];
    }
  }
  if (part == 0) {
    a.logp_out[i] = acc ? lp : lp0;
    a.accept[i] = acc ? 1.f : 0.f;
    a.dH[i] = dH;
  }
}

template <int C, int LPR, int R>
void launch_family(const HmcArgs& a, int family, hipStream_t stream) {
  const dim3 grid((unsigned)(((long)a.B + R - 1) / R)), block(hmc_threads(R, LPR));
  if (family == glm::FAM_BERNOULLI)
    hipLaunchKernelGGL((glm_hmc_kernel<C, LPR, glm::FAM_BERNOULLI, R>), grid, block, 0, stream, a);
  else if (family == glm::FAM_POISSON)
    hipLaunchKernelGGL((glm_hmc_kernel<C, LPR, glm::FAM_POISSON, R>), grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL((glm_hmc_kernel<C, LPR, glm::FAM_GAUSSIAN, R>), grid, block, 0, stream, a);
  NF_HIP_CHECK(hipGetLastError());
}

template <int C, int LPR>
void launch_rows(const HmcArgs& a, int family, int rows, hipStream_t stream) {
  if (rows == 128) launch_family<C, LPR, 128>(a, family, stream);
  else if (rows == 64) launch_family<C, LPR, 64>(a, family, stream);
  else launch_family<C, LPR, 32>(a, family, stream);
}

}  // namespace
}  // namespace nf

using namespace nf;

int nf_glm_hmc_rows(int B, int D, int rows) {
  if (rows == 128 || rows == 64 || rows == 32) return rows;
  if (rows != 0) return -1;
  // whichever tile measured fastest per (B, D) band on one MI355X (docs/PERF_NOTES.md, "HMC
  // trajectory"): D > 16 runs 2 or 4 lanes per chain and wants the full 128 rows; the narrow
  // widths want 64, 32 at D > 8 while the grid is small, and 128 once B alone fills the card
  if (D > 16 || B >= 262144) return 128;
  if (D > 8 && B <= 4096) return 32;
  return 64;
}

void nf_launch_glm_hmc_trajectory(const float* theta0, long ldt, const float* p0,
                                  const float* logp0, const float* grad0, const float* eps,
                                  const float* minv, const float* log_u, int L, const float* X,
                                  long ldx, const float* y, const float* prec_dev, float prec_host,
                                  int has_prior, int family, float inv_var, float scale, int rows,
                                  float* theta_prop, float* p_prop, float* theta_out,
                                  float* logp_out, float* grad_out, float* accept, float* dH,
                                  int B, int N, int D, hipStream_t stream) {
  if (B <= 0 || N <= 0) return;
  const HmcArgs a{theta0, p0, logp0, grad0, eps, minv, log_u, X, y, ldt, ldx,
                  glm::Prior{prec_dev, prec_host, has_prior}, inv_var, scale, theta_prop, p_prop,
                  theta_out, logp_out, grad_out, accept, dH, B, N, D, L};
  const int R = nf_glm_hmc_rows(B, D, rows);
  if (D <= 1) launch_rows<1, 1>(a, family, R, stream);
  else if (D <= 2) launch_rows<2, 1>(a, family, R, stream);
  else if (D <= 4) launch_rows<4, 1>(a, family, R, stream);
  else if (D <= 8) launch_rows<8, 1>(a, family, R, stream);
  else if (D <= 16) launch_rows<16, 1>(a, family, R, stream);
  else if (D <= 32) launch_rows<16, 2>(a, family, R, stream);
  else launch_rows<16, 4>(a, family, R, stream);
}
