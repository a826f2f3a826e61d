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
// element-wise frame of elementwise_flow.h; the element mathematics is dsf_elem.h (shared with the
// degree sweep of dsf_sweep.hip); this file holds its Op.
#include "dsf_elem.h"

namespace nf {

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
