// Element mathematics of the rational-quadratic spline (Durkan et al. 2019): the knot
// derivative, the bin search over the two softmaxes, the position in the bin with the spline
// there (forward, or the closed-form quadratic of the inverse) and the gradients of one element.
// Shared by the element-wise kernels of spline.hip and the degree sweep of rqs_sweep.hip;
// __host__ __device__, so a host program can exercise it too. See spline.hip for the layout and
// the parametrisation.
//
// EW_EXP / EW_LOG / EW_RCP / EW_SQRT are the macros of elementwise_flow.h: the fast device
// intrinsics, or the accurate library forms in a unit that defines EW_ACCURATE_MATH before its
// first include.
#pragma once

#include "elementwise_flow.h"

namespace nf {

constexpr float RQS_MIN = 1e-3f;            // min_w = min_h = min_d
constexpr float RQS_C0 = 0.539742417236952f;  // log(expm1(1 - min_d)): ud = 0 gives d = 1
constexpr float RQS_Q = 0.631752495386337f;   // 1 - exp(-(1 - min_d)) = sigmoid(c0)

// Interior derivative d = min_d + softplus(ud + c0). Around ud = 0 it is evaluated as the equal
// 1 + log((1 - q) + q e^ud), which is exactly 1 at ud = 0 (q + (1 - q) == 1 in fp32, exp(0) == 1,
// log(1) == 0, with the fast intrinsics too): a d one ulp off 1 rounds every element's
// log dy/dx of the identity spline the same way, and the row sum drifts by Dh ulp. Its absolute
// error (~1e-7) would be a relative one where d approaches min_d, so far below 0 (rare) the
// literal form with the precise log1p is used.
EW_HD float rqs_deriv(float ud) {
  if (ud > -2.0f && ud < 15.0f) return 1.0f + EW_LOG(fmaf(RQS_Q, EW_EXP(ud), 1.0f - RQS_Q));
  const float t = ud + RQS_C0;
  return RQS_MIN + (t > 20.f ? t : log1pf(EW_EXP(t)));
}

// The bin that holds one element, and what the backward needs of the two softmaxes.
struct RqsBin {
  int k;               // bin index: number of interior knots <= v
  float xk, w, yk, h;  // lower knot and size of the bin, in x and in y
  float sw, sh;        // the bin's softmax values (widths, heights)
  float cw, ch;        // softmax mass of the bins before it
  float u0, u1;        // ud + c0 at the bin's two knots (unused at an end knot)
  float d0, d1;        // derivatives at the bin's two knots
};

// Loads the width and height planes of element j of a row (pr = its params row), leaves the two
// softmaxes in smw / smh (0 for k >= K) and picks the bin of v: by the x-knots, or by the
// y-knots for the inverse. The knots are running sums from -bound, as in the composite.
template <int KMAX, bool INVERSE, typename TP>
EW_HD void rqs_find_bin(const TP* __restrict__ pr, unsigned j, unsigned Dh, int K, float bound,
                        float v, float (&smw)[KMAX], float (&smh)[KMAX], RqsBin& bn) {
  // all 2K loads are issued before the first use; the column offset walks plane by plane
  unsigned ow = j, oh = j + (unsigned)K * Dh;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < K) {
      smw[k] = ew_ld(pr, ow);
      smh[k] = ew_ld(pr, oh);
      ow += Dh;
      oh += Dh;
    } else {
      smw[k] = 0.f;
      smh[k] = 0.f;
    }
  }
  float mw = -INFINITY, mh = -INFINITY;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < K) {
      mw = fmaxf(mw, smw[k]);
      mh = fmaxf(mh, smh[k]);
    }
  }
  float sw = 0.f, sh = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < K) {
      smw[k] = EW_EXP(smw[k] - mw);
      smh[k] = EW_EXP(smh[k] - mh);
      sw += smw[k];
      sh += smh[k];
    }
  }
  const float iw = EW_RCP(sw), ih = EW_RCP(sh);
  const float c2 = 2.0f * bound, cm = 1.0f - (float)K * RQS_MIN;
  float kx = -bound, ky = -bound, cw = 0.f, ch = 0.f;
  bn.k = 0;
  bn.xk = bn.yk = -bound;
  bn.sw = bn.sh = bn.cw = bn.ch = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < K) {
      smw[k] *= iw;
      smh[k] *= ih;
      const float wk = c2 * fmaf(cm, smw[k], RQS_MIN);
      const float hk = c2 * fmaf(cm, smh[k], RQS_MIN);
      // the knots increase, so the last bin whose lower knot is <= v is the bin of v
      const bool take = k == 0 || v >= (INVERSE ? ky : kx);
      bn.k = take ? k : bn.k;
      bn.xk = take ? kx : bn.xk;
      bn.sw = take ? smw[k] : bn.sw;
      bn.yk = take ? ky : bn.yk;
      bn.sh = take ? smh[k] : bn.sh;
      bn.cw = take ? cw : bn.cw;
      bn.ch = take ? ch : bn.ch;
      kx += wk;
      ky += hk;
      cw += smw[k];
      ch += smh[k];
    }
  }
  bn.w = c2 * fmaf(cm, bn.sw, RQS_MIN);
  bn.h = c2 * fmaf(cm, bn.sh, RQS_MIN);
  // end knots have derivative 1; the index is clamped so the gather stays inside the planes
  const bool first = bn.k == 0, last = bn.k == K - 1;
  const float ud0 = ew_ld(pr, (unsigned)(2 * K + (first ? 0 : bn.k - 1)) * Dh + j);
  const float ud1 = ew_ld(pr, (unsigned)(2 * K + (last ? K - 2 : bn.k)) * Dh + j);
  bn.u0 = ud0 + RQS_C0;
  bn.u1 = ud1 + RQS_C0;
  bn.d0 = first ? 1.0f : rqs_deriv(ud0);
  bn.d1 = last ? 1.0f : rqs_deriv(ud1);
}

// Position in the bin and the spline there. s = h / w is a true division: with equal width
// and height (zero params) it is exactly 1, and then so are den and P: the identity spline's
// ldj is exactly 0 instead of a rounding bias that adds up over a row.
struct RqsEval {
  float rw, s, e, th, t1, den, rden, P;
};

template <bool INVERSE>
EW_HD void rqs_eval(const RqsBin& bn, float v, RqsEval& ev) {
  ev.rw = EW_RCP(bn.w);
  ev.s = bn.h / bn.w;
  ev.e = bn.d1 + bn.d0 - 2.0f * ev.s;
  if (INVERSE) {
    const float dl = v - bn.yk;
    const float a = fmaf(bn.h, ev.s - bn.d0, dl * ev.e);
    const float b = fmaf(bn.h, bn.d0, -dl * ev.e);
    const float c = -ev.s * dl;
    const float disc = fmaxf(fmaf(b, b, -4.0f * a * c), 0.f);
    ev.th = 2.0f * c * EW_RCP(-b - EW_SQRT(disc));
  } else {
    ev.th = (v - bn.xk) * ev.rw;
  }
  ev.t1 = ev.th * (1.0f - ev.th);
  ev.den = fmaf(ev.e, ev.t1, ev.s);
  ev.rden = EW_RCP(ev.den);
  // P = d1 th^2 + 2 s th (1 - th) + d0 (1 - th)^2 as s + (d1 - s) th^2 + (d0 - s) (1 - th)^2:
  // with d0 = d1 = s (the identity spline) P, den and log dy/dx are exact
  const float om = 1.0f - ev.th;
  ev.P = fmaf(bn.d1 - ev.s, ev.th * ev.th, fmaf(bn.d0 - ev.s, om * om, ev.s));
}

// Gradients of one element. With theta = (x - xk) / w, s = h / w, t1 = theta (1 - theta),
//   N = s theta^2 + d0 t1,  den = s + e t1,  e = d0 + d1 - 2 s,  y = yk + h N / den,
//   P = d1 theta^2 + 2 s t1 + d0 (1 - theta)^2,  L = log y' = 2 log s + log P - 2 log den,
// the upstream pair (ge on y, le on L) is pushed to (theta, s, h, yk, d0, d1) and from there to
// (x, xk, w, h, yk). The inverse direction enters with ge = -(g - gl L_x) / y', le = -gl.
struct RqsGrad {
  float gin;               // gradient of the direction's input
  float Gw, Gxk, Gh, Gyk;  // gradients of the bin's width / lower x-knot / height / lower y-knot
  float gu0, gu1;          // gradients of ud at the bin's two knots (0 at an end knot)
};

template <bool INVERSE>
EW_HD void rqs_grad_elem(const RqsBin& bn, const RqsEval& ev, int K, float g, float gl,
                         RqsGrad& gr) {
  const float th = ev.th, t1 = ev.t1, s = ev.s, rden = ev.rden, rP = EW_RCP(ev.P);
  const float om = 1.0f - th, om2 = 1.0f - 2.0f * th;
  const float N = th * fmaf(s - bn.d0, th, bn.d0);
  const float hr2 = bn.h * rden * rden;
  const float ypr = s * s * ev.P * rden * rden;
  // partials of L
  const float P_th = 2.0f * (bn.d1 * th + s * om2 - bn.d0 * om);
  const float L_th = P_th * rP - 2.0f * ev.e * om2 * rden;
  const float L_s = 2.0f * EW_RCP(s) + 2.0f * t1 * rP - 2.0f * (1.0f - 2.0f * t1) * rden;
  const float L_d0 = om * om * rP - 2.0f * t1 * rden;
  const float L_d1 = th * th * rP - 2.0f * t1 * rden;
  // partials of y
  const float y_th = bn.w * ypr;
  const float y_s = hr2 * (th * th * ev.den - N * (1.0f - 2.0f * t1));
  const float y_h = N * rden;
  const float y_d0 = hr2 * t1 * (ev.den - N);
  const float y_d1 = -hr2 * N * t1;
  float ge = g, le = gl;
  if (INVERSE) {
    ge = -(g - gl * L_th * ev.rw) * EW_RCP(ypr);
    le = -gl;
  }
  const float A_th = ge * y_th + le * L_th;
  const float A_s = ge * y_s + le * L_s;
  gr.gin = INVERSE ? -ge : A_th * ev.rw;
  gr.Gxk = -A_th * ev.rw;
  gr.Gw = -(A_th * th + A_s * s) * ev.rw;
  gr.Gh = ge * y_h + A_s * ev.rw;
  gr.Gyk = ge;
  // d = min_d + softplus(u): dd/dud = sigmoid(u)
  const float sg0 = EW_RCP(1.0f + EW_EXP(-bn.u0)), sg1 = EW_RCP(1.0f + EW_EXP(-bn.u1));
  gr.gu0 = bn.k == 0 ? 0.f : (ge * y_d0 + le * L_d0) * sg0;
  gr.gu1 = bn.k == K - 1 ? 0.f : (ge * y_d1 + le * L_d1) * sg1;
}

}  // namespace nf
