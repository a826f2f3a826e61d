// Deep sigmoidal flow transformer (Huang et al. 2018, "Neural Autoregressive Flows"): fused
// forward / inverse and their backward for gfx950.
//
// Layout (see vi_normflows_amd/ops/reference.py dsf_transform for the math):
//   params [B, 3H*D]  conditioner output, fp32 or bf16, PLANE-major: column p*D + j is plane p of
//                     element j; planes [0,H) ua (slopes), [H,2H) b (shifts), [2H,3H) uw (mixture
//                     logits). Adjacent lanes read adjacent columns of one plane, so every plane
//                     load is coalesced.
//   x      [B, D]     fp32 input of the direction taken (the inverse reads y here)
//   y      [B, D]     fp32 output
//   ldj    [B]        fp32 sum_j log dy/dx (inverse: minus that, at the recovered x)
//
// One wave64 owns one row; 4 rows per 256-thread block; lanes stride over j; ldj is a 64-wide
// shuffle sum, so there are no atomics and every result is bitwise repeatable.
//
// An element's H units live in registers: the kernels are templated on HMAX in {8, 16, 32} and
// every loop over units is fully unrolled and predicated on the wave-uniform h < H. Everything is
// evaluated in log space (three logsumexps over the units), so |x| of 1e4 and widely spread
// logits neither overflow nor lose the small mixture terms. The mixture logits enter relative to
// their maximum and the softmax normaliser Z is subtracted from the logarithm of each sum, so
// with zero params log s is exactly logsigmoid(x) and y = x up to one rounding.
//
// The inverse has no closed form: y lies between min_j p_j and max_j p_j, so the root lies in
// [min_j (y - b_j) / a_j, max_j (y - b_j) / a_j], and DSF_BISECT bisections of that bracket (a
// compile-time trip count, no data-dependent exit: a NaN cannot spin a wave) bring it to fp32
// resolution; ldj is then evaluated at the recovered x.
//
// The backward saves nothing: it recomputes the units from params and the x-side value (the
// input of the forward direction, the output of the inverse direction), and one body serves both
// because x = f^-1(y) gives dx/dy = 1 / y', dx/dp = -f_p / y' and ldj_inv = -L(x, p) with the
// same partials f_p, y', L_x, L_p.
#include "nf_common.h"

#include <math.h>

// The element math is __host__ __device__ so it can also be exercised by a host program; the
// fast intrinsics exist on the device only.
#if defined(__HIP_DEVICE_COMPILE__)
#define DSF_EXP(v) __expf(v)
#define DSF_LOG(v) __logf(v)
#define DSF_RCP(v) __builtin_amdgcn_rcpf(v)
#else
#define DSF_EXP(v) expf(v)
#define DSF_LOG(v) logf(v)
#define DSF_RCP(v) (1.0f / (v))
#endif
#define DSF_HD __host__ __device__ __forceinline__

namespace nf {

constexpr float DSF_C0 = 0.541324854612918f;   // log(e - 1): ua = 0 gives a = 1
constexpr float DSF_Q = 0.632120558828558f;    // 1 - 1/e = sigmoid(c0)
constexpr float DSF_A_MIN = 1.17549435e-38f;   // slopes are kept normal: log a and 1 / a finite
constexpr int DSF_BISECT = 40;                 // halvings of the inverse's bracket

DSF_HD float dsf_ld(const float* p, unsigned j) { return p[j]; }
DSF_HD float dsf_ld(const bf16_t* p, unsigned j) {
  union { uint32_t u; float f; } c;
  c.u = ((uint32_t)p[j]) << 16;
  return c.f;
}
DSF_HD void dsf_st(float* p, unsigned j, float v) { p[j] = v; }
DSF_HD void dsf_st(bf16_t* p, unsigned j, float v) {
  const __hip_bfloat16 h = __float2bfloat16(v);
  p[j] = *reinterpret_cast<const bf16_t*>(&h);
}

// Slope a = softplus(ua + c0). Around ua = 0 it is evaluated as the equal
// 1 + log((1 - q) + q e^ua), which is exactly 1 at ua = 0 (as rqs_deriv in spline.hip); its
// absolute error would be a relative one where a approaches 0, so far below 0 the literal form
// with the precise log1p is used.
DSF_HD float dsf_slope(float ua) {
  if (ua > -2.0f && ua < 15.0f) return 1.0f + DSF_LOG(fmaf(DSF_Q, DSF_EXP(ua), 1.0f - DSF_Q));
  const float t = ua + DSF_C0;
  return fmaxf(t > 20.f ? t : log1pf(DSF_EXP(t)), DSF_A_MIN);
}

// The H units of one element: slopes, shifts, mixture logits relative to their maximum
// (entries h >= H are never read: every loop is predicated) and the softmax normaliser
// Z = log sum_h exp(lw_h).
template <int HMAX>
struct DsfUnits {
  float a[HMAX], b[HMAX], lw[HMAX];
  float Z;
};

template <int HMAX, typename TP>
DSF_HD void dsf_load(const TP* __restrict__ pr, unsigned j, unsigned D, int H, DsfUnits<HMAX>& u) {
  // all 3H loads are issued before the first use; the column offset walks plane by plane
  unsigned oa = j, ob = j + (unsigned)H * D, ow = j + 2u * (unsigned)H * D;
#pragma unroll
  for (int h = 0; h < HMAX; ++h) {
    if (h < H) {
      u.a[h] = dsf_ld(pr, oa);
      u.b[h] = dsf_ld(pr, ob);
      u.lw[h] = dsf_ld(pr, ow);
      oa += D;
      ob += D;
      ow += D;
    } else {
      u.a[h] = 1.f;
      u.b[h] = 0.f;
      u.lw[h] = 0.f;
    }
  }
  float m = -INFINITY;
#pragma unroll
  for (int h = 0; h < HMAX; ++h)
    if (h < H) m = fmaxf(m, u.lw[h]);
  float s = 0.f;
#pragma unroll
  for (int h = 0; h < HMAX; ++h) {
    if (h < H) {
      u.a[h] = dsf_slope(u.a[h]);
      u.lw[h] -= m;
      s += DSF_EXP(u.lw[h]);
    }
  }
  u.Z = DSF_LOG(s);
}

// logsigmoid(p) and logsigmoid(-p) from one exp and one log.
DSF_HD void dsf_logsig(float p, float& lsp, float& lsn) {
  const float l1 = DSF_LOG(1.0f + DSF_EXP(-fabsf(p)));
  lsp = fminf(p, 0.f) - l1;
  lsn = fminf(-p, 0.f) - l1;
}

// y(x) alone, for the bisection: log s - log(1 - s) with both logsumexps shifted by their maxima.
template <int HMAX>
DSF_HD float dsf_value(const DsfUnits<HMAX>& u, int H, float x) {
  float A[HMAX], Bn[HMAX];
  float mA = -INFINITY, mB = -INFINITY;
#pragma unroll
  for (int h = 0; h < HMAX; ++h) {
    if (h < H) {
      float lsp, lsn;
      dsf_logsig(fmaf(u.a[h], x, u.b[h]), lsp, lsn);
      A[h] = u.lw[h] + lsp;
      Bn[h] = u.lw[h] + lsn;
      mA = fmaxf(mA, A[h]);
      mB = fmaxf(mB, Bn[h]);
    }
  }
  float sA = 0.f, sB = 0.f;
#pragma unroll
  for (int h = 0; h < HMAX; ++h) {
    if (h < H) {
      sA += DSF_EXP(A[h] - mA);
      sB += DSF_EXP(Bn[h] - mB);
    }
  }
  return (mA + (DSF_LOG(sA) - u.Z)) - (mB + (DSF_LOG(sB) - u.Z));
}

// The three logsumexps at x. A / Bn / C leave as the normalised terms
//   al_h = w_h sig_h / s,  be_h = w_h (1 - sig_h) / (1 - s),  ga_h = w_h a_h sig_h (1 - sig_h) / s'
// (each sums to 1 over h), which are all the backward needs.
template <int HMAX>
struct DsfEval {
  float A[HMAX], Bn[HMAX], C[HMAX];
  float logs, log1ms, y, L;   // L = log dy/dx
};

template <int HMAX>
DSF_HD void dsf_eval(const DsfUnits<HMAX>& u, int H, float x, DsfEval<HMAX>& ev) {
  float mA = -INFINITY, mB = -INFINITY, mC = -INFINITY;
#pragma unroll
  for (int h = 0; h < HMAX; ++h) {
    if (h < H) {
      float lsp, lsn;
      dsf_logsig(fmaf(u.a[h], x, u.b[h]), lsp, lsn);
      ev.A[h] = u.lw[h] + lsp;
      ev.Bn[h] = u.lw[h] + lsn;
      ev.C[h] = (u.lw[h] + DSF_LOG(u.a[h])) + (lsp + lsn);
      mA = fmaxf(mA, ev.A[h]);
      mB = fmaxf(mB, ev.Bn[h]);
      mC = fmaxf(mC, ev.C[h]);
    } else {
      ev.A[h] = ev.Bn[h] = ev.C[h] = 0.f;
    }
  }
  float sA = 0.f, sB = 0.f, sC = 0.f;
#pragma unroll
  for (int h = 0; h < HMAX; ++h) {
    if (h < H) {
      ev.A[h] = DSF_EXP(ev.A[h] - mA);
      ev.Bn[h] = DSF_EXP(ev.Bn[h] - mB);
      ev.C[h] = DSF_EXP(ev.C[h] - mC);
      sA += ev.A[h];
      sB += ev.Bn[h];
      sC += ev.C[h];
    }
  }
  const float rA = DSF_RCP(sA), rB = DSF_RCP(sB), rC = DSF_RCP(sC);
#pragma unroll
  for (int h = 0; h < HMAX; ++h) {
    if (h < H) {
      ev.A[h] *= rA;
      ev.Bn[h] *= rB;
      ev.C[h] *= rC;
    }
  }
  // with zero params log sA == log sC == Z bit for bit, and the differences vanish
  ev.logs = mA + (DSF_LOG(sA) - u.Z);
  ev.log1ms = mB + (DSF_LOG(sB) - u.Z);
  ev.y = ev.logs - ev.log1ms;
  ev.L = (mC - ev.logs - ev.log1ms) + (DSF_LOG(sC) - u.Z);
}

// The x with y(x) = v: DSF_BISECT halvings of the closed-form bracket. Every comparison with a
// NaN is false, so a NaN only moves one end; the trip count is fixed.
template <int HMAX>
DSF_HD float dsf_solve(const DsfUnits<HMAX>& u, int H, float v) {
  float lo = INFINITY, hi = -INFINITY;
#pragma unroll
  for (int h = 0; h < HMAX; ++h) {
    if (h < H) {
      const float r = (v - u.b[h]) / u.a[h];
      lo = fminf(lo, r);
      hi = fmaxf(hi, r);
    }
  }
#pragma unroll 1
  for (int it = 0; it < DSF_BISECT; ++it) {
    const float mid = 0.5f * lo + 0.5f * hi;
    const bool below = dsf_value<HMAX>(u, H, mid) < v;
    lo = below ? mid : lo;
    hi = below ? hi : mid;
  }
  return 0.5f * lo + 0.5f * hi;
}

// One element of the forward / inverse transform; returns the output and adds log dy/dx
// (inverse: minus it, at the recovered x) to acc.
template <int HMAX, bool INVERSE, typename TP>
DSF_HD float dsf_fwd_elem(const TP* __restrict__ pr, unsigned j, unsigned D, int H, float v,
                          float& acc) {
  DsfUnits<HMAX> u;
  dsf_load<HMAX>(pr, j, D, H, u);
  const float x = INVERSE ? dsf_solve<HMAX>(u, H, v) : v;
  DsfEval<HMAX> ev;
  dsf_eval<HMAX>(u, H, x, ev);
  if (INVERSE) {
    acc -= ev.L;
    return x;
  }
  acc += ev.L;
  return ev.y;
}

template <int HMAX, bool INVERSE, typename TP>
__global__ void __launch_bounds__(256) dsf_fwd_kernel(
    const TP* __restrict__ params, const float* __restrict__ x, float* __restrict__ y,
    float* __restrict__ ldj, int B, int D, int H, int ldj_init) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const TP* p_r = params + row * (long)(3 * H) * D;
  const float* x_r = x + row * D;
  float* y_r = y + row * D;
  float acc = 0.f;
#pragma unroll 1
  for (int j = lane; j < D; j += 64)
    y_r[j] = dsf_fwd_elem<HMAX, INVERSE>(p_r, j, (unsigned)D, H, x_r[j], acc);
  acc = wave_sum(acc);
  if (lane == 0) ldj[row] = ldj_init ? acc : ldj[row] + acc;
}

// Backward of element j of a row at its x-side value: writes its 3H parameter gradients
// (dpr = the dparams row) and returns the gradient of the direction's input. With
// sig_h = sigmoid(p_h) and the normalised terms of DsfEval,
//   dy/dp_h = al_h (1 - sig_h) + be_h sig_h,      dy/dlw_h = al_h - be_h,
//   dL/dp_h = ga_h (1 - 2 sig_h) - al_h (1 - sig_h) + be_h sig_h,
//   dL/dlw_h = ga_h - al_h - be_h,                dL/dlog a_h = ga_h  (besides p_h = a_h x + b_h);
// lw = log softmax(uw) turns G_h into G_h - w_h sum_k G_k = G_h + w_h le, and
// da/dua = sigmoid(ua + c0). The inverse direction enters with ge = -(g - gl L_x) / y', le = -gl.
template <int HMAX, bool INVERSE, typename TP>
DSF_HD float dsf_bwd_elem(const TP* __restrict__ pr, TP* __restrict__ dpr, unsigned j,
                          unsigned D, int H, float x, float g, float gl) {
  DsfUnits<HMAX> u;
  dsf_load<HMAX>(pr, j, D, H, u);
  DsfEval<HMAX> ev;
  dsf_eval<HMAX>(u, H, x, ev);
  float sg[HMAX];
  float Lx = 0.f;
#pragma unroll
  for (int h = 0; h < HMAX; ++h) {
    if (h < H) {
      const float p = fmaf(u.a[h], x, u.b[h]);
      const float e = DSF_EXP(-fabsf(p));
      const float r = DSF_RCP(1.0f + e);
      sg[h] = p >= 0.f ? r : e * r;
      const float om = p >= 0.f ? e * r : r;
      Lx = fmaf(u.a[h], ev.C[h] * (om - sg[h]) - ev.A[h] * om + ev.Bn[h] * sg[h], Lx);
    } else {
      sg[h] = 0.f;
    }
  }
  float ge = g, le = gl;
  if (INVERSE) {
    ge = -(g - gl * Lx) * DSF_EXP(-ev.L);
    le = -gl;
  }
  const float s = DSF_EXP(ev.logs), s1 = DSF_EXP(ev.log1ms);
  float gin = 0.f;
  unsigned oa = j, ob = j + (unsigned)H * D, ow = j + 2u * (unsigned)H * D;
#pragma unroll
  for (int h = 0; h < HMAX; ++h) {
    if (h < H) {
      const float al = ev.A[h], be = ev.Bn[h], ga = ev.C[h], om = 1.0f - sg[h];
      const float yp = al * om + be * sg[h];
      const float Lp = ga * (om - sg[h]) - al * om + be * sg[h];
      const float Gp = ge * yp + le * Lp;
      gin = fmaf(Gp, u.a[h], gin);
      const float t = dsf_ld(pr, oa) + DSF_C0;
      const float da = DSF_RCP(1.0f + DSF_EXP(-t));
      dsf_st(dpr, oa, fmaf(Gp, x, le * ga * DSF_RCP(u.a[h])) * da);
      dsf_st(dpr, ob, Gp);
      const float w = fmaf(al, s, be * s1);
      dsf_st(dpr, ow, ge * (al - be) + le * (ga - al - be + w));
      oa += D;
      ob += D;
      ow += D;
    }
  }
  return INVERSE ? -ge : gin;
}

// g_out [B, D], g_ldj [B]: upstream gradients of the direction's output and ldj.
// dparams [B, 3H D] in the dtype of params (every column written), gx [B, D].
template <int HMAX, bool INVERSE, typename TP>
__global__ void __launch_bounds__(256) dsf_bwd_kernel(
    const TP* __restrict__ params, const float* __restrict__ x, const float* __restrict__ g_out,
    const float* __restrict__ g_ldj, TP* __restrict__ dparams, float* __restrict__ gx, int B,
    int D, int H) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const long prow = row * (long)(3 * H) * D;
  const float gl = g_ldj[row];
#pragma unroll 1
  for (int j = lane; j < D; j += 64)
    gx[row * D + j] = dsf_bwd_elem<HMAX, INVERSE>(params + prow, dparams + prow, j, (unsigned)D,
                                                  H, x[row * D + j], g_out[row * D + j], gl);
}

}  // namespace nf

using namespace nf;

// columns inside a params row are 32-bit offsets (byte offsets stay below 2^31)
static bool dsf_row_fits(int H, int D) { return (long)(3 * H) * D < (1L << 29); }

#define NF_DSF_HMAX(CALL)           \
  do {                              \
    if (H <= 8) { CALL(8); }        \
    else if (H <= 16) { CALL(16); } \
    else { CALL(32); }              \
  } while (0)

void nf_launch_dsf_fwd(const void* params, int params_is_bf16, const float* x, float* y,
                       float* ldj, int B, int D, int H, int inverse, int ldj_init,
                       hipStream_t stream) {
  if (B <= 0 || D <= 0) return;
  if (H < 1 || H > 32 || !dsf_row_fits(H, D)) {
    fprintf(stderr, "dsf_fwd: need 1 <= H <= 32 and 3H D < 2^29\n");
    abort();
  }
  dim3 grid((B + 3) / 4), block(256);
#define NF_DSF_F(HM)                                                                          \
  do {                                                                                        \
    if (params_is_bf16) {                                                                     \
      if (inverse)                                                                            \
        hipLaunchKernelGGL((dsf_fwd_kernel<HM, true, bf16_t>), grid, block, 0, stream,         \
                           (const bf16_t*)params, x, y, ldj, B, D, H, ldj_init);              \
      else                                                                                    \
        hipLaunchKernelGGL((dsf_fwd_kernel<HM, false, bf16_t>), grid, block, 0, stream,        \
                           (const bf16_t*)params, x, y, ldj, B, D, H, ldj_init);              \
    } else {                                                                                  \
      if (inverse)                                                                            \
        hipLaunchKernelGGL((dsf_fwd_kernel<HM, true, float>), grid, block, 0, stream,          \
                           (const float*)params, x, y, ldj, B, D, H, ldj_init);               \
      else                                                                                    \
        hipLaunchKernelGGL((dsf_fwd_kernel<HM, false, float>), grid, block, 0, stream,         \
                           (const float*)params, x, y, ldj, B, D, H, ldj_init);               \
    }                                                                                         \
  } while (0)
  NF_DSF_HMAX(NF_DSF_F);
#undef NF_DSF_F
  NF_HIP_CHECK(hipGetLastError());
}

void nf_launch_dsf_bwd(const void* params, int params_is_bf16, const float* x, const float* g_out,
                       const float* g_ldj, void* dparams, float* gx, int B, int D, int H,
                       int inverse, hipStream_t stream) {
  if (B <= 0 || D <= 0) return;
  if (H < 1 || H > 32 || !dsf_row_fits(H, D)) {
    fprintf(stderr, "dsf_bwd: need 1 <= H <= 32 and 3H D < 2^29\n");
    abort();
  }
  dim3 grid((B + 3) / 4), block(256);
#define NF_DSF_B(HM)                                                                          \
  do {                                                                                        \
    if (params_is_bf16) {                                                                     \
      if (inverse)                                                                            \
        hipLaunchKernelGGL((dsf_bwd_kernel<HM, true, bf16_t>), grid, block, 0, stream,         \
                           (const bf16_t*)params, x, g_out, g_ldj, (bf16_t*)dparams, gx, B,   \
                           D, H);                                                             \
      else                                                                                    \
        hipLaunchKernelGGL((dsf_bwd_kernel<HM, false, bf16_t>), grid, block, 0, stream,        \
                           (const bf16_t*)params, x, g_out, g_ldj, (bf16_t*)dparams, gx, B,   \
                           D, H);                                                             \
    } else {                                                                                  \
      if (inverse)                                                                            \
        hipLaunchKernelGGL((dsf_bwd_kernel<HM, true, float>), grid, block, 0, stream,          \
                           (const float*)params, x, g_out, g_ldj, (float*)dparams, gx, B, D,  \
                           H);                                                                \
      else                                                                                    \
        hipLaunchKernelGGL((dsf_bwd_kernel<HM, false, float>), grid, block, 0, stream,         \
                           (const float*)params, x, g_out, g_ldj, (float*)dparams, gx, B, D,  \
                           H);                                                                \
    }                                                                                         \
  } while (0)
  NF_DSF_HMAX(NF_DSF_B);
#undef NF_DSF_B
  NF_HIP_CHECK(hipGetLastError());
}
