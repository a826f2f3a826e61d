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
//
// The kernels, the row accessors, the fast-math macros and the launch dispatch are the shared
// element-wise frame of elementwise_flow.h; this file holds the element mathematics and its Op.
#include "elementwise_flow.h"

namespace nf {

constexpr float DSF_C0 = 0.541324854612918f;   // log(e - 1): ua = 0 gives a = 1
constexpr float DSF_Q = 0.632120558828558f;    // 1 - 1/e = sigmoid(c0)
constexpr float DSF_A_MIN = 1.17549435e-38f;   // slopes are kept normal: log a and 1 / a finite
constexpr int DSF_BISECT = 40;                 // halvings of the inverse's bracket

// Slope a = softplus(ua + c0). Around ua = 0 it is evaluated as the equal
// 1 + log((1 - q) + q e^ua), which is exactly 1 at ua = 0 (as rqs_deriv in spline.hip); its
// absolute error would be a relative one where a approaches 0, so far below 0 the literal form
// with the precise log1p is used.
EW_HD float dsf_slope(float ua) {
  if (ua > -2.0f && ua < 15.0f) return 1.0f + EW_LOG(fmaf(DSF_Q, EW_EXP(ua), 1.0f - DSF_Q));
  const float t = ua + DSF_C0;
  return fmaxf(t > 20.f ? t : log1pf(EW_EXP(t)), DSF_A_MIN);
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
EW_HD void dsf_load(const TP* __restrict__ pr, unsigned j, unsigned D, int H, DsfUnits<HMAX>& u) {
  // all 3H loads are issued before the first use; the column offset walks plane by plane
  unsigned oa = j, ob = j + (unsigned)H * D, ow = j + 2u * (unsigned)H * D;
#pragma unroll
  for (int h = 0; h < HMAX; ++h) {
    if (h < H) {
      u.a[h] = ew_ld(pr, oa);
      u.b[h] = ew_ld(pr, ob);
      u.lw[h] = ew_ld(pr, ow);
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
      s += EW_EXP(u.lw[h]);
    }
  }
  u.Z = EW_LOG(s);
}

// logsigmoid(p) and logsigmoid(-p) from one exp and one log.
EW_HD void dsf_logsig(float p, float& lsp, float& lsn) {
  const float l1 = EW_LOG(1.0f + EW_EXP(-fabsf(p)));
  lsp = fminf(p, 0.f) - l1;
  lsn = fminf(-p, 0.f) - l1;
}

// y(x) alone, for the bisection: log s - log(1 - s) with both logsumexps shifted by their maxima.
template <int HMAX>
EW_HD float dsf_value(const DsfUnits<HMAX>& u, int H, float x) {
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
      sA += EW_EXP(A[h] - mA);
      sB += EW_EXP(Bn[h] - mB);
    }
  }
  return (mA + (EW_LOG(sA) - u.Z)) - (mB + (EW_LOG(sB) - u.Z));
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
EW_HD void dsf_eval(const DsfUnits<HMAX>& u, int H, float x, DsfEval<HMAX>& ev) {
  float mA = -INFINITY, mB = -INFINITY, mC = -INFINITY;
#pragma unroll
  for (int h = 0; h < HMAX; ++h) {
    if (h < H) {
      float lsp, lsn;
      dsf_logsig(fmaf(u.a[h], x, u.b[h]), lsp, lsn);
      ev.A[h] = u.lw[h] + lsp;
      ev.Bn[h] = u.lw[h] + lsn;
      ev.C[h] = (u.lw[h] + EW_LOG(u.a[h])) + (lsp + lsn);
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
      ev.A[h] = EW_EXP(ev.A[h] - mA);
      ev.Bn[h] = EW_EXP(ev.Bn[h] - mB);
      ev.C[h] = EW_EXP(ev.C[h] - mC);
      sA += ev.A[h];
      sB += ev.Bn[h];
      sC += ev.C[h];
    }
  }
  const float rA = EW_RCP(sA), rB = EW_RCP(sB), rC = EW_RCP(sC);
#pragma unroll
  for (int h = 0; h < HMAX; ++h) {
    if (h < H) {
      ev.A[h] *= rA;
      ev.Bn[h] *= rB;
      ev.C[h] *= rC;
    }
  }
  // with zero params log sA == log sC == Z bit for bit, and the differences vanish
  ev.logs = mA + (EW_LOG(sA) - u.Z);
  ev.log1ms = mB + (EW_LOG(sB) - u.Z);
  ev.y = ev.logs - ev.log1ms;
  ev.L = (mC - ev.logs - ev.log1ms) + (EW_LOG(sC) - u.Z);
}

// The x with y(x) = v: DSF_BISECT halvings of the closed-form bracket. Every comparison with a
// NaN is false, so a NaN only moves one end; the trip count is fixed.
template <int HMAX>
EW_HD float dsf_solve(const DsfUnits<HMAX>& u, int H, float v) {
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

// The sigmoidal flow as an element-wise Op (elementwise_flow.h): H sigmoid units. Its backward
// takes the x-side value in both directions (the inverse's output). The element functions are
// its members themselves: a member that only forwarded to a free function would add an inlining
// layer, and that alone reorders the generated code.
template <int HMAX, bool INVERSE>
struct DsfOp {
  int H;
  static constexpr const char* NEED = "1 <= H <= 32";
  EW_HD bool valid() const { return H >= 1 && H <= 32; }
  EW_HD int planes() const { return 3 * H; }

  // One element of the forward / inverse transform; returns the output and adds log dy/dx
  // (inverse: minus it, at the recovered x) to acc.
  template <typename TP>
  EW_HD float fwd_elem(const TP* __restrict__ pr, unsigned j, unsigned D, float v,
                       float& acc) const {
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

  // Backward of element j of a row at its x-side value: writes its 3H parameter gradients
  // (dpr = the dparams row) and returns the gradient of the direction's input. With
  // sig_h = sigmoid(p_h) and the normalised terms of DsfEval,
  //   dy/dp_h = al_h (1 - sig_h) + be_h sig_h,      dy/dlw_h = al_h - be_h,
  //   dL/dp_h = ga_h (1 - 2 sig_h) - al_h (1 - sig_h) + be_h sig_h,
  //   dL/dlw_h = ga_h - al_h - be_h,               dL/dlog a_h = ga_h  (besides p_h = a_h x + b_h);
  // lw = log softmax(uw) turns G_h into G_h - w_h sum_k G_k = G_h + w_h le, and
  // da/dua = sigmoid(ua + c0). The inverse direction enters with ge = -(g - gl L_x) / y', le = -gl.
  template <typename TP>
  EW_HD float bwd_elem(const TP* __restrict__ pr, TP* __restrict__ dpr, unsigned j, unsigned D,
                       float x, float g, float gl) const {
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
        const float e = EW_EXP(-fabsf(p));
        const float r = EW_RCP(1.0f + e);
        sg[h] = p >= 0.f ? r : e * r;
        const float om = p >= 0.f ? e * r : r;
        Lx = fmaf(u.a[h], ev.C[h] * (om - sg[h]) - ev.A[h] * om + ev.Bn[h] * sg[h], Lx);
      } else {
        sg[h] = 0.f;
      }
    }
    float ge = g, le = gl;
    if (INVERSE) {
      ge = -(g - gl * Lx) * EW_EXP(-ev.L);
      le = -gl;
    }
    const float s = EW_EXP(ev.logs), s1 = EW_EXP(ev.log1ms);
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
        const float t = ew_ld(pr, oa) + DSF_C0;
        const float da = EW_RCP(1.0f + EW_EXP(-t));
        ew_st(dpr, oa, fmaf(Gp, x, le * ga * EW_RCP(u.a[h])) * da);
        ew_st(dpr, ob, Gp);
        const float w = fmaf(al, s, be * s1);
        ew_st(dpr, ow, ge * (al - be) + le * (ga - al - be + w));
        oa += D;
        ob += D;
        ow += D;
      }
    }
    return INVERSE ? -ge : gin;
  }
};

}  // namespace nf

using namespace nf;

void nf_launch_dsf_fwd(const void* params, int params_is_bf16, const float* x, float* y,
                       float* ldj, int B, int D, int H, int inverse, int ldj_init,
                       hipStream_t stream) {
  ew_launch<DsfOp>("dsf_fwd", EwFwd{x, y, ldj, ldj_init}, params, params_is_bf16, B, D, inverse,
                   stream, H);
}

void nf_launch_dsf_bwd(const void* params, int params_is_bf16, const float* x, const float* g_out,
                       const float* g_ldj, void* dparams, float* gx, int B, int D, int H,
                       int inverse, hipStream_t stream) {
  ew_launch<DsfOp>("dsf_bwd", EwBwd{x, g_out, g_ldj, dparams, gx}, params, params_is_bf16, B, D,
                   inverse, stream, H);
}
