// Rational-quadratic spline coupling transform (Durkan et al. 2019, "Neural Spline Flows"):
// fused forward / inverse and their backward for gfx950.
//
// Layout (see vi_normflows_amd/ops/reference.py rqs_transform for the math):
//   params [B, (3K-1)*Dh]  conditioner output, fp32 or bf16, PLANE-major: column p*Dh + j is
//                          plane p of element j; planes [0,K) unnormalised widths, [K,2K)
//                          heights, [2K,3K-1) interior derivatives. Adjacent lanes read adjacent
//                          columns of one plane, so every plane load is coalesced.
//   x      [B, Dh]         fp32 input of the direction taken (the inverse reads y here)
//   y      [B, Dh]         fp32 output
//   ldj    [B]             fp32 sum_j log dy/dx (inverse: minus that, at the recovered x)
//
// One wave64 owns one row; 4 rows per 256-thread block; lanes stride over j; ldj is a 64-wide
// shuffle sum, so there are no atomics and every result is bitwise repeatable.
//
// An element's two softmaxes live in registers: the kernels are templated on KMAX in
// {8, 16, 32}, every loop over bins is fully unrolled and predicated on the wave-uniform k < K,
// and the bin is picked with conditional moves while the knots are accumulated (a runtime-indexed
// per-thread array would go to scratch). Only the two derivatives that bound the chosen bin are
// needed, so they are gathered by index instead of loading all K-1 planes into registers.
//
// The backward saves nothing: it recomputes the bin from params and the input-side value, in
// both directions, and one body serves both because x = f^-1(y) gives dx/dy = 1 / y',
// dx/dp = -f_p / y' and ldj_inv = -L(x, p) with the same partials f_p, y', L_x, L_p.
//
// The kernels, the row accessors, the fast-math macros and the launch dispatch are the shared
// element-wise frame of elementwise_flow.h; the element mathematics is rqs_elem.h (shared with
// the degree sweep of rqs_sweep.hip) and this file holds its Op.
#include "rqs_elem.h"

namespace nf {

// The spline as an element-wise Op (elementwise_flow.h): K bins on (-bound, bound). The element
// functions are its members themselves: a member that only forwarded to a free function would
// add an inlining layer, and that alone reorders the generated code.
template <int KMAX, bool INVERSE>
struct RqsOp {
  int K;
  float bound;
  static constexpr const char* NEED = "2 <= K <= 32, bound > 0";
  EW_HD bool valid() const { return K >= 2 && K <= 32 && bound > 0.f; }
  EW_HD int planes() const { return 3 * K - 1; }

  // One element of the forward / inverse transform; returns the output and adds log dy/dx
  // (inverse: minus it) to acc.
  template <typename TP>
  EW_HD float fwd_elem(const TP* __restrict__ pr, unsigned j, unsigned Dh, float v,
                       float& acc) const {
    if (!(v > -bound && v < bound)) return v;   // linear tails (and NaN): identity, ldj 0
    float smw[KMAX], smh[KMAX];
    RqsBin bn;
    rqs_find_bin<KMAX, INVERSE>(pr, j, Dh, K, bound, v, smw, smh, bn);
    RqsEval ev;
    rqs_eval<INVERSE>(bn, v, ev);
    const float ypr = ev.s * ev.s * ev.P * ev.rden * ev.rden;   // dy/dx
    const float L = EW_LOG(ypr);
    float out;
    if (INVERSE) {
      out = fmaf(ev.th, bn.w, bn.xk);
      acc -= L;
    } else {
      // s th^2 + d0 th (1 - th) = th (d0 + (s - d0) th)
      out = fmaf(bn.h * ev.th * fmaf(ev.s - bn.d0, ev.th, bn.d0), ev.rden, bn.yk);
      acc += L;
    }
    return out;
  }

  // Backward of element j of a row: writes its 3K-1 parameter gradients (dpr = the dparams row)
  // and returns the gradient of the direction's input.
  template <typename TP>
  EW_HD float bwd_elem(const TP* __restrict__ pr, TP* __restrict__ dpr, unsigned j, unsigned Dh,
                       float v, float g, float gl) const {
    if (!(v > -bound && v < bound)) {   // tails: identity, no parameter gradient
      unsigned o = j;
      for (int k = 0; k < 3 * K - 1; ++k, o += Dh) ew_st(dpr, o, 0.f);
      return g;
    }
    float smw[KMAX], smh[KMAX];
    RqsBin bn;
    rqs_find_bin<KMAX, INVERSE>(pr, j, Dh, K, bound, v, smw, smh, bn);
    RqsEval ev;
    rqs_eval<INVERSE>(bn, v, ev);
    RqsGrad gr;
    rqs_grad_elem<INVERSE>(bn, ev, K, g, gl, gr);
    // A bin's size gets Gw (Gh) if it is the chosen bin and the knot's gradient if it lies
    // before it; then the softmax Jacobian sm_i (G_i - sum_j G_j sm_j) times d size / d softmax.
    const float cs = 2.0f * bound * (1.0f - (float)K * RQS_MIN);
    const float Sw = fmaf(gr.Gw, bn.sw, gr.Gxk * bn.cw);
    const float Sh = fmaf(gr.Gh, bn.sh, gr.Gyk * bn.ch);
    unsigned ow = j, oh = j + (unsigned)K * Dh, od = j + 2u * (unsigned)K * Dh;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < K) {
        const float Gwk = k == bn.k ? gr.Gw : (k < bn.k ? gr.Gxk : 0.f);
        const float Ghk = k == bn.k ? gr.Gh : (k < bn.k ? gr.Gyk : 0.f);
        ew_st(dpr, ow, cs * smw[k] * (Gwk - Sw));
        ew_st(dpr, oh, cs * smh[k] * (Ghk - Sh));
        ow += Dh;
        oh += Dh;
      }
    }
#pragma unroll
    for (int k = 0; k < KMAX - 1; ++k) {
      if (k < K - 1) {
        const float gd = k == bn.k - 1 ? gr.gu0 : (k == bn.k ? gr.gu1 : 0.f);
        ew_st(dpr, od, gd);
        od += Dh;
      }
    }
    return gr.gin;
  }
};

}  // namespace nf

using namespace nf;

void nf_launch_rqs_fwd(const void* params, int params_is_bf16, const float* x, float* y,
                       float* ldj, int B, int Dh, int K, float bound, int inverse, int ldj_init,
                       hipStream_t stream) {
  ew_launch<RqsOp>("rqs_fwd", EwFwd{x, y, ldj, ldj_init}, params, params_is_bf16, B, Dh, inverse,
                   stream, K, bound);
}

void nf_launch_rqs_bwd(const void* params, int params_is_bf16, const float* x, const float* g_out,
                       const float* g_ldj, void* dparams, float* gx, int B, int Dh, int K,
                       float bound, int inverse, hipStream_t stream) {
  ew_launch<RqsOp>("rqs_bwd", EwBwd{x, g_out, g_ldj, dparams, gx}, params, params_is_bf16, B, Dh,
                   inverse, stream, K, bound);
}

