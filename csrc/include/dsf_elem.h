// Element mathematics of the deep sigmoidal flow (Huang et al. 2018): the units of one element,
// y(x), the three logsumexps with log dy/dx, and the root solve of the inverse. Shared by the
// element-wise kernels of dsf.hip and the degree sweep of dsf_sweep.hip; __host__ __device__, so a
// host program can exercise it too. See dsf.hip for the layout and the parametrisation.
//
// EW_EXP / EW_LOG / EW_RCP are the macros of elementwise_flow.h: the fast device intrinsics, or
// the accurate library forms in a unit that defines EW_ACCURATE_MATH before its first include.
#pragma once

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

// The closed-form bracket of the x with y(x) = v: y lies between min_h p_h and max_h p_h, so the
// root lies in [min_h (v - b_h) / a_h, max_h (v - b_h) / a_h].
template <int HMAX>
EW_HD void dsf_bracket(const DsfUnits<HMAX>& u, int H, float v, float& lo, float& hi) {
  lo = INFINITY;
  hi = -INFINITY;
#pragma unroll
  for (int h = 0; h < HMAX; ++h) {
    if (h < H) {
      const float r = (v - u.b[h]) / u.a[h];
      lo = fminf(lo, r);
      hi = fmaxf(hi, r);
    }
  }
}

// The x with y(x) = v: DSF_BISECT halvings of the closed-form bracket. Every comparison with a
// NaN is false, so a NaN only moves one end; the trip count is fixed. (The bracket is written out
// here: going through dsf_bracket adds an inlining layer that reorders the element-wise kernels.)
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

}  // namespace nf
