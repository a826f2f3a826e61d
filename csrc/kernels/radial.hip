// Fused K-layer radial flow stack, forward + backward (gfx950).
//
//   f(z) = z + beta h(r) (z - z0),   r = ||z - z0||,   h = 1 / (alpha + r)
//   log|det J| = (D-1) log(1 + beta h) + log(1 + beta alpha h^2)
// (Rezende & Mohamed 2015, Sec. 3.2; named but never implemented in the reference,
//  normflows/normflows/flows.py:1.)  alpha > 0 and beta >= -alpha are enforced by the
// caller's reparameterisation (softplus), so the map is invertible.
// Same row mapping / per-row gradient scheme as planar.hip.
#include "nf_common.h"

namespace nf {

template <bool WROW>
__device__ __forceinline__ float rsum_r(float v) {
  if (WROW) return wave_sum(v);
  return v;
}

struct RadialArgs {
  const float* z;
  const float* Z0;     // [K][D] or [K][N][D]
  const float* AL;     // alpha [K] or [K][N]
  const float* BE;     // beta  [K] or [K][N]
  float* zK;
  float* ldj;
  float* saved;        // [K][N][D]
  const float* gz;
  const float* gl;
  float* dz;
  float* dZ0;          // [K][N][D]
  float* dA;           // [K][N]
  float* dBe;          // [K][N]
  int N, D, K, per_sample;
};

template <bool WROW, int PER>
__global__ void __launch_bounds__(256) radial_fwd_kernel(RadialArgs a) {
  const int lane = threadIdx.x & 63;
  const long row = WROW ? (((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6)
                        : ((long)blockIdx.x * blockDim.x + threadIdx.x);
  if (row >= a.N) return;
  const int D = a.D;
  float z[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = WROW ? lane + 64 * i : i;
    z[i] = j < D ? a.z[row * D + j] : 0.f;
  }
  float ldj = 0.f;
  for (int k = 0; k < a.K; ++k) {
    const long pb = a.per_sample ? ((long)k * a.N + row) * D : (long)k * D;
    const long sb = a.per_sample ? (long)k * a.N + row : k;
    const float al = a.AL[sb], be = a.BE[sb];
    float d[PER];
    float rr = 0.f;
    float* sv = a.saved + ((long)k * a.N + row) * D;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int j = WROW ? lane + 64 * i : i;
      d[i] = j < D ? z[i] - a.Z0[pb + j] : 0.f;
      if (j < D) sv[j] = z[i];
      rr += d[i] * d[i];
    }
    rr = rsum_r<WROW>(rr);
    const float r = sqrtf(rr);
    const float h = 1.f / (al + r);
    const float bh = be * h;
#pragma unroll
    for (int i = 0; i < PER; ++i) z[i] += bh * d[i];
    ldj += (float)(D - 1) * __logf(fabsf(1.f + bh)) + __logf(fabsf(1.f + be * al * h * h));
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = WROW ? lane + 64 * i : i;
    if (j < D) a.zK[row * D + j] = z[i];
  }
  if (!WROW || lane == 0) a.ldj[row] = ldj;
}

template <bool WROW, int PER>
__global__ void __launch_bounds__(256) radial_bwd_kernel(RadialArgs a) {
  const int lane = threadIdx.x & 63;
  const long row = WROW ? (((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6)
                        : ((long)blockIdx.x * blockDim.x + threadIdx.x);
  if (row >= a.N) return;
  const int D = a.D;
  const float Dm1 = (float)(D - 1);
  float g[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = WROW ? lane + 64 * i : i;
    g[i] = j < D ? a.gz[row * D + j] : 0.f;
  }
  const float c = a.gl[row];
  for (int k = a.K - 1; k >= 0; --k) {
    const long pb = a.per_sample ? ((long)k * a.N + row) * D : (long)k * D;
    const long sb = a.per_sample ? (long)k * a.N + row : k;
    const float al = a.AL[sb], be = a.BE[sb];
    const float* sv = a.saved + ((long)k * a.N + row) * D;
    float d[PER];
    float rr = 0.f, gd = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int j = WROW ? lane + 64 * i : i;
      d[i] = j < D ? sv[j] - a.Z0[pb + j] : 0.f;
      rr += d[i] * d[i];
      gd += g[i] * d[i];
    }
    rr = rsum_r<WROW>(rr);
    gd = rsum_r<WROW>(gd);
    const float r = sqrtf(rr);
    const float ir = r > 1e-20f ? 1.f / r : 0.f;
    const float h = 1.f / (al + r);
    const float h2 = h * h;
    const float bh = be * h;
    const float q1 = 1.f + bh;            // (D-1) log q1
    const float q2 = 1.f + be * al * h2;  // log q2
    // dldj/dr = -(D-1) beta h^2 / q1 - 2 beta alpha h^3 / q2
    const float dldj_dr = -Dm1 * be * h2 / q1 - 2.f * be * al * h2 * h / q2;
    // coefficient on d in dL/dz beyond (1 + beta h) g
    const float coef_d = -be * h2 * gd * ir + c * dldj_dr * ir;
    const float dbe = gd * h + c * (Dm1 * h / q1 + al * h2 / q2);
    const float dal = -be * h2 * gd + c * (-Dm1 * be * h2 / q1 + be * h2 * (1.f - 2.f * al * h) / q2);
    float* dZr = a.dZ0 + ((long)k * a.N + row) * D;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int j = WROW ? lane + 64 * i : i;
      const float via_d = bh * g[i] + coef_d * d[i];   // dL/dd (excluding the identity path)
      if (j < D) dZr[j] = -via_d;
      g[i] = g[i] + via_d;
    }
    if (!WROW || lane == 0) {
      a.dA[(long)k * a.N + row] = dal;
      a.dBe[(long)k * a.N + row] = dbe;
    }
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = WROW ? lane + 64 * i : i;
    if (j < D) a.dz[row * D + j] = g[i];
  }
}

// ---- inverse ----
// With d = y - z0 and r' = ||d|| the preimage radius r >= 0 solves r (1 + beta h(r)) = r', i.e.
// r^2 + q r - alpha r' = 0, q = alpha + beta - r' (alpha > 0, beta >= -alpha: one root >= 0).
// The root is taken without cancellation for either sign of q; then x = z0 + d / (1 + beta h)
// and the log-det is minus the forward's at x. a.z = y, a.zK = x, a.saved[k] = the preimage
// under layer k (what the forward kernel saves as that layer's input).
template <bool WROW, int PER>
__global__ void __launch_bounds__(256) radial_inv_kernel(RadialArgs a) {
  const int lane = threadIdx.x & 63;
  const long row = WROW ? (((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6)
                        : ((long)blockIdx.x * blockDim.x + threadIdx.x);
  if (row >= a.N) return;
  const int D = a.D;
  float z[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = WROW ? lane + 64 * i : i;
    z[i] = j < D ? a.z[row * D + j] : 0.f;
  }
  float ldj = 0.f;
  for (int k = a.K - 1; k >= 0; --k) {
    const long pb = a.per_sample ? ((long)k * a.N + row) * D : (long)k * D;
    const long sb = a.per_sample ? (long)k * a.N + row : k;
    const float al = a.AL[sb], be = a.BE[sb];
    float d[PER], z0[PER];
    float rr = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int j = WROW ? lane + 64 * i : i;
      z0[i] = j < D ? a.Z0[pb + j] : 0.f;
      d[i] = j < D ? z[i] - z0[i] : 0.f;
      rr += d[i] * d[i];
    }
    rr = rsum_r<WROW>(rr);
    const float rp = sqrtf(rr);
    const float q = al + be - rp;
    const float disc = sqrtf(q * q + 4.f * al * rp);
    const float r = q > 0.f ? 2.f * al * rp / (q + disc) : 0.5f * (disc - q);
    const float h = 1.f / (al + r);
    const float bh = be * h;
    const float iq1 = 1.f / (1.f + bh);
    float* sv = a.saved + ((long)k * a.N + row) * D;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int j = WROW ? lane + 64 * i : i;
      z[i] = z0[i] + d[i] * iq1;
      if (j < D) sv[j] = z[i];
    }
    ldj -= (float)(D - 1) * __logf(fabsf(1.f + bh)) + __logf(fabsf(1.f + be * al * h * h));
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = WROW ? lane + 64 * i : i;
    if (j < D) a.zK[row * D + j] = z[i];
  }
  if (!WROW || lane == 0) a.ldj[row] = ldj;
}

// Backward of the inverse: a.gz = dLoss/dx, a.gl = dLoss/dldj, layers 0 .. K-1. With x = saved[k],
// e = x - z0, r = ||e||, J = dy/dx = q1 I - beta h^2 e e^T / r (symmetric, q1 = 1 + beta h,
// q2 = 1 + beta alpha h^2) and Lf the forward log-det term at x:
//   gbar = gx - gL dLf/dx,                 dLf/dx = dLf/dr e / r
//   v = J^-1 gbar = (gbar + beta h^2 (e.gbar) e / (r q2)) / q1,         gy = v
//   gz0 = (J - I) v + gL dLf/dx,  gbeta = -h (e.v) - gL dLf/dbeta,
//   galpha = beta h^2 (e.v) - gL dLf/dalpha
template <bool WROW, int PER>
__global__ void __launch_bounds__(256) radial_inv_bwd_kernel(RadialArgs a) {
  const int lane = threadIdx.x & 63;
  const long row = WROW ? (((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6)
                        : ((long)blockIdx.x * blockDim.x + threadIdx.x);
  if (row >= a.N) return;
  const int D = a.D;
  const float Dm1 = (float)(D - 1);
  float g[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = WROW ? lane + 64 * i : i;
    g[i] = j < D ? a.gz[row * D + j] : 0.f;
  }
  const float c = a.gl[row];
  for (int k = 0; k < a.K; ++k) {
    const long pb = a.per_sample ? ((long)k * a.N + row) * D : (long)k * D;
    const long sb = a.per_sample ? (long)k * a.N + row : k;
    const float al = a.AL[sb], be = a.BE[sb];
    const float* sv = a.saved + ((long)k * a.N + row) * D;
    float e[PER];
    float rr = 0.f, ge = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int j = WROW ? lane + 64 * i : i;
      e[i] = j < D ? sv[j] - a.Z0[pb + j] : 0.f;
      rr += e[i] * e[i];
      ge += g[i] * e[i];
    }
    rr = rsum_r<WROW>(rr);
    ge = rsum_r<WROW>(ge);
    const float r = sqrtf(rr);
    const float ir = r > 1e-20f ? 1.f / r : 0.f;
    const float h = 1.f / (al + r);
    const float h2 = h * h;
    const float bh = be * h;
    const float q1 = 1.f + bh;
    const float q2 = 1.f + be * al * h2;
    // gL dLf/dx = dldr e
    const float dldr = c * (-Dm1 * be * h2 / q1 - 2.f * be * al * h2 * h / q2) * ir;
    const float egb = ge - dldr * rr;                        // e.gbar
    const float ke = be * h2 * ir / q2 * egb;
    const float iq1 = 1.f / q1;
    const float ev = (egb + ke * rr) * iq1;                  // e.v
    const float coef = -be * h2 * ev * ir + dldr;
    float* dZr = a.dZ0 + ((long)k * a.N + row) * D;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int j = WROW ? lane + 64 * i : i;
      g[i] = (g[i] + (ke - dldr) * e[i]) * iq1;              // v
      if (j < D) dZr[j] = bh * g[i] + coef * e[i];
    }
    if (!WROW || lane == 0) {
      a.dA[(long)k * a.N + row] =
          be * h2 * ev - c * (-Dm1 * be * h2 / q1 + be * h2 * (1.f - 2.f * al * h) / q2);
      a.dBe[(long)k * a.N + row] = -h * ev - c * (Dm1 * h / q1 + al * h2 / q2);
    }
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = WROW ? lane + 64 * i : i;
    if (j < D) a.dz[row * D + j] = g[i];
  }
}

enum RadialKind { kRadialFwd, kRadialBwd, kRadialInv, kRadialInvBwd };

template <bool WROW, int PER>
static void launch_radial(const RadialArgs& a, RadialKind bwd, hipStream_t stream) {
  const long threads = WROW ? (long)a.N * 64 : (long)a.N;
  dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  if (bwd == kRadialBwd)
    hipLaunchKernelGGL((radial_bwd_kernel<WROW, PER>), grid, block, 0, stream, a);
  else if (bwd == kRadialInv)
    hipLaunchKernelGGL((radial_inv_kernel<WROW, PER>), grid, block, 0, stream, a);
  else if (bwd == kRadialInvBwd)
    hipLaunchKernelGGL((radial_inv_bwd_kernel<WROW, PER>), grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL((radial_fwd_kernel<WROW, PER>), grid, block, 0, stream, a);
  NF_HIP_CHECK(hipGetLastError());
}

static void dispatch_radial(const RadialArgs& a, RadialKind bwd, hipStream_t stream) {
  const int D = a.D;
  if (D <= 2) return launch_radial<false, 2>(a, bwd, stream);
  if (D <= 4) return launch_radial<false, 4>(a, bwd, stream);
  if (D <= 8) return launch_radial<false, 8>(a, bwd, stream);
  if (D <= 16) return launch_radial<false, 16>(a, bwd, stream);
  if (D <= 64) return launch_radial<true, 1>(a, bwd, stream);
  if (D <= 128) return launch_radial<true, 2>(a, bwd, stream);
  if (D <= 256) return launch_radial<true, 4>(a, bwd, stream);
  if (D <= 512) return launch_radial<true, 8>(a, bwd, stream);
  return launch_radial<true, 16>(a, bwd, stream);
}

}  // namespace nf

using namespace nf;

void nf_launch_radial_fwd(const float* z, const float* Z0, const float* AL, const float* BE,
                          float* zK, float* ldj, float* saved, int N, int D, int K,
                          int per_sample, hipStream_t stream) {
  if (N <= 0) return;
  RadialArgs a{};
  a.z = z; a.Z0 = Z0; a.AL = AL; a.BE = BE; a.zK = zK; a.ldj = ldj; a.saved = saved;
  a.N = N; a.D = D; a.K = K; a.per_sample = per_sample;
  dispatch_radial(a, kRadialFwd, stream);
}

void nf_launch_radial_bwd(const float* saved, const float* Z0, const float* AL, const float* BE,
                          const float* gz, const float* gl, float* dz, float* dZ0, float* dA,
                          float* dBe, int N, int D, int K, int per_sample, hipStream_t stream) {
  if (N <= 0) return;
  RadialArgs a{};
  a.saved = (float*)saved; a.Z0 = Z0; a.AL = AL; a.BE = BE; a.gz = gz; a.gl = gl; a.dz = dz;
  a.dZ0 = dZ0; a.dA = dA; a.dBe = dBe;
  a.N = N; a.D = D; a.K = K; a.per_sample = per_sample;
  dispatch_radial(a, kRadialBwd, stream);
}

void nf_launch_radial_inv(const float* y, const float* Z0, const float* AL, const float* BE,
                          float* x, float* ldj, float* saved, int N, int D, int K,
                          int per_sample, hipStream_t stream) {
  if (N <= 0) return;
  RadialArgs a{};
  a.z = y; a.Z0 = Z0; a.AL = AL; a.BE = BE; a.zK = x; a.ldj = ldj; a.saved = saved;
  a.N = N; a.D = D; a.K = K; a.per_sample = per_sample;
  dispatch_radial(a, kRadialInv, stream);
}

void nf_launch_radial_inv_bwd(const float* saved, const float* Z0, const float* AL,
                              const float* BE, const float* gx, const float* gl, float* dy,
                              float* dZ0, float* dA, float* dBe, int N, int D, int K,
                              int per_sample, hipStream_t stream) {
  if (N <= 0) return;
  RadialArgs a{};
  a.saved = (float*)saved; a.Z0 = Z0; a.AL = AL; a.BE = BE; a.gz = gx; a.gl = gl; a.dz = dy;
  a.dZ0 = dZ0; a.dA = dA; a.dBe = dBe;
  a.N = N; a.D = D; a.K = K; a.per_sample = per_sample;
  dispatch_radial(a, kRadialInvBwd, stream);
}
