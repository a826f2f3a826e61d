// TORCH_LIBRARY fragment for the autoregressive degree sweeps: MAF sampling and the IAF inverse
// (made_sweep.hip), the inverse of a MADE-conditioned DSF layer (dsf_sweep.hip) and the sequential
// direction of a MADE-conditioned spline layer (rqs_sweep.hip) in one masked pass, and the adjoint
// sweep all three share (sweep_adjoint.hip). The ops themselves are not differentiable; the
// implicit gradient is assembled in ops/autoregressive.py.
#include <torch/library.h>
#include <ATen/ATen.h>

#include "bind_common.h"
#include "launchers.h"

namespace {

// fp32 GPU [rows, cols] with unit inner stride; returns the row stride in elements
long mat_stride(const char* op, const at::Tensor& t, const char* n, int64_t rows, int64_t cols,
                const at::Device& dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev, op, ": ", n, " must be on the device of v");
  TORCH_CHECK(t.scalar_type() == at::kFloat, op, ": ", n, " must be fp32, got ",
              t.scalar_type());
  TORCH_CHECK(t.dim() == 2 && t.size(0) == rows && t.size(1) == cols, op, ": ", n,
              " has shape ", t.sizes(), ", expected [", rows, ", ", cols, "]");
  TORCH_CHECK(cols == 1 || t.stride(1) == 1, op, ": ", n, " must have unit inner stride");
  const int64_t rs = rows > 1 ? t.stride(0) : cols;
  TORCH_CHECK(rs >= cols, op, ": ", n, " has overlapping rows (row stride ", rs, ")");
  return (long)rs;
}

void chk_vec(const char* op, const at::Tensor& t, const char* n, int64_t numel, at::ScalarType st,
             const at::Device& dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev && t.scalar_type() == st && t.is_contiguous() &&
                  t.numel() == numel,
              op, ": ", n, " must be a contiguous ", st, " tensor of ", numel,
              " elements on the device of v");
}

// The checks and the launch struct both sweeps share; the output layer has out_mult rows per
// coordinate. The LDS-budget check is the caller's (it depends on the kernel).
NfMadeSweep sweep_args(const char* op, const at::Tensor& v, at::TensorList weights,
                       at::TensorList biases, const at::Tensor& perm, const at::Tensor& ubeg,
                       int64_t out_mult, const c10::optional<at::Tensor>& ctx_bias,
                       const at::Tensor& x, const at::Tensor& ldj) {
  TORCH_CHECK(v.is_cuda() && v.dim() == 2, op, ": v must be a GPU tensor [B, D]");
  const int64_t L = (int64_t)weights.size() - 1;
  TORCH_CHECK(L >= 1 && L <= NF_MADE_SWEEP_MAX_HIDDEN && biases.size() == weights.size(),
              op, ": need 1 .. ", NF_MADE_SWEEP_MAX_HIDDEN,
              " hidden layers plus the output layer, one bias per weight");
  TORCH_CHECK(weights[0].dim() == 2, op, ": a hidden weight must be a matrix");
  const int64_t B = v.size(0), D = v.size(1), H = weights[0].size(0);
  TORCH_CHECK(B >= 1 && B < (int64_t(1) << 31) && D >= 1 && H >= 1 && D < (1 << 24) &&
                  H < (1 << 24),
              op, ": bad sizes B = ", B, ", D = ", D, ", H = ", H);
  const auto dev = v.device();
  NfMadeSweep s{};
  s.B = (int)B; s.D = (int)D; s.H = (int)H; s.L = (int)L;
  s.ldv = mat_stride(op, v, "v", B, D, dev);
  s.v = v.data_ptr<float>();
  for (int64_t l = 0; l < L; ++l) {
    s.ldw[l] = mat_stride(op, weights[l], "a hidden weight", H, l == 0 ? D : H, dev);
    s.W[l] = weights[l].data_ptr<float>();
    chk_vec(op, biases[l], "a hidden bias", H, at::kFloat, dev);
    s.b[l] = biases[l].data_ptr<float>();
  }
  s.ldo = mat_stride(op, weights[L], "the output weight", out_mult * D, H, dev);
  s.Wo = weights[L].data_ptr<float>();
  chk_vec(op, biases[L], "the output bias", out_mult * D, at::kFloat, dev);
  s.bo = biases[L].data_ptr<float>();
  chk_vec(op, perm, "perm", D, at::kInt, dev);
  chk_vec(op, ubeg, "ubeg", L * (D + 2), at::kInt, dev);
  s.perm = perm.data_ptr<int>();
  s.ubeg = ubeg.data_ptr<int>();
  if (ctx_bias.has_value() && ctx_bias->defined()) {
    s.ldc = mat_stride(op, *ctx_bias, "ctx_bias", B, H, dev);
    s.ctx = ctx_bias->data_ptr<float>();
  }
  s.ldx = mat_stride(op, x, "x", B, D, dev);
  s.x = x.data_ptr<float>();
  chk_vec(op, ldj, "ldj", B, at::kFloat, dev);
  s.ldj = ldj.data_ptr<float>();
  return s;
}

void made_sweep(const at::Tensor& v, at::TensorList weights, at::TensorList biases,
                const at::Tensor& perm, const at::Tensor& ubeg, int64_t kind, double param,
                const c10::optional<at::Tensor>& ctx_bias, const at::Tensor& x,
                const at::Tensor& ldj) {
  TORCH_CHECK(kind >= 0 && kind <= 2,
              "made_sweep: unknown kind ", kind, " (0 maf_sample, 1 iaf_gated, 2 iaf_affine)");
  NfMadeSweep s = sweep_args("made_sweep", v, weights, biases, perm, ubeg, 2, ctx_bias, x, ldj);
  TORCH_CHECK(nf_made_sweep_rows(s.D, s.H, s.L) > 0, "made_sweep: (D, H, L) = (", s.D, ", ", s.H,
              ", ", s.L, ") exceeds the kernel's LDS budget (made_sweep_supported)");
  s.kind = (int)kind;
  s.param = (float)param;
  nf_launch_made_sweep(s, cur_stream());
}

// y [B, D] -> z = x, ldj of the inverse of a DSF layer with `units` sigmoid units per coordinate;
// the output layer is [3 units D, H] plane-major (MADE(out_mult = 3 units)).
void dsf_sweep(const at::Tensor& y, at::TensorList weights, at::TensorList biases,
               const at::Tensor& perm, const at::Tensor& ubeg, int64_t units,
               const c10::optional<at::Tensor>& ctx_bias, const at::Tensor& x,
               const at::Tensor& ldj) {
  TORCH_CHECK(units >= 1 && units <= 32, "dsf_sweep: need 1 <= units <= 32, got ", units);
  NfMadeSweep s =
      sweep_args("dsf_sweep", y, weights, biases, perm, ubeg, 3 * units, ctx_bias, x, ldj);
  TORCH_CHECK(nf_dsf_sweep_rows(s.D, s.H, s.L, (int)units) > 0, "dsf_sweep: (D, H, L, U) = (", s.D,
              ", ", s.H, ", ", s.L, ", ", units,
              ") exceeds the kernel's LDS budget (dsf_sweep_supported)");
  nf_launch_dsf_sweep(s, (int)units, cur_stream());
}

// y [B, D] -> z = x with T(z) = y, ldj of the inverse of a spline layer with `bins` bins on
// (-bound, bound); the output layer is [(3 bins - 1) D, H] plane-major (MADE(out_mult = 3 bins - 1)).
void rqs_sweep(const at::Tensor& y, at::TensorList weights, at::TensorList biases,
               const at::Tensor& perm, const at::Tensor& ubeg, int64_t bins, double bound,
               const c10::optional<at::Tensor>& ctx_bias, const at::Tensor& x,
               const at::Tensor& ldj) {
  TORCH_CHECK(bins >= 2 && bins <= 32, "rqs_sweep: need 2 <= bins <= 32, got ", bins);
  TORCH_CHECK(bound > 0 && (float)bound > 0.f, "rqs_sweep: need bound > 0, got ", bound);
  NfMadeSweep s =
      sweep_args("rqs_sweep", y, weights, biases, perm, ubeg, 3 * bins - 1, ctx_bias, x, ldj);
  TORCH_CHECK(nf_rqs_sweep_rows(s.D, s.H, s.L, (int)bins) > 0, "rqs_sweep: (D, H, L, K) = (", s.D,
              ", ", s.H, ", ", s.L, ", ", bins,
              ") exceeds the kernel's LDS budget (rqs_sweep_supported)");
  nf_launch_rqs_sweep(s, (int)bins, (float)bound, cur_stream());
}

// rows per block for (D, H, L); 0 when the shape does not fit
int64_t made_sweep_rows(int64_t D, int64_t H, int64_t L) {
  if (D < 1 || H < 1 || L < 1 || D >= (1 << 24) || H >= (1 << 24) || L > NF_MADE_SWEEP_MAX_HIDDEN)
    return 0;
  return nf_made_sweep_rows((int)D, (int)H, (int)L);
}

bool made_sweep_supported(int64_t D, int64_t H, int64_t L) { return made_sweep_rows(D, H, L) > 0; }

// rows per block for (D, H, L, U); 0 when the shape does not fit or U is out of range
int64_t dsf_sweep_rows(int64_t D, int64_t H, int64_t L, int64_t U) {
  if (D < 1 || H < 1 || L < 1 || D >= (1 << 24) || H >= (1 << 24) ||
      L > NF_MADE_SWEEP_MAX_HIDDEN || U < 1 || U > 32)
    return 0;
  return nf_dsf_sweep_rows((int)D, (int)H, (int)L, (int)U);
}

bool dsf_sweep_supported(int64_t D, int64_t H, int64_t L, int64_t U) {
  return dsf_sweep_rows(D, H, L, U) > 0;
}

// rows per block for (D, H, L, K); 0 when the shape does not fit or K is out of range
int64_t rqs_sweep_rows(int64_t D, int64_t H, int64_t L, int64_t K) {
  if (D < 1 || H < 1 || L < 1 || D >= (1 << 24) || H >= (1 << 24) ||
      L > NF_MADE_SWEEP_MAX_HIDDEN || K < 2 || K > 32)
    return 0;
  return nf_rqs_sweep_rows((int)D, (int)H, (int)L, (int)K);
}

bool rqs_sweep_supported(int64_t D, int64_t H, int64_t L, int64_t K) {
  return rqs_sweep_rows(D, H, L, K) > 0;
}

// The adjoint of the degree sweeps (sweep_adjoint.hip): gx, d [B, D]; q, c [B, D, P]
// coordinate-major; hidden [l] [B, H] the activations at the solution; weights the L hidden layers
// then the output layer [P D, H] plane-major. Writes w [B, D], pbar [B, D, P] (may be c) and
// a[l] [B, H].
void sweep_adjoint(const at::Tensor& gx, const at::Tensor& d, const at::Tensor& q,
                   const at::Tensor& c, at::TensorList hidden, at::TensorList weights,
                   const at::Tensor& perm, const at::Tensor& ubeg, const at::Tensor& w,
                   const at::Tensor& pbar, at::TensorList a) {
  const char* op = "sweep_adjoint";
  TORCH_CHECK(gx.is_cuda() && gx.dim() == 2, op, ": gx must be a GPU tensor [B, D]");
  const int64_t L = (int64_t)weights.size() - 1;
  TORCH_CHECK(L >= 1 && L <= NF_MADE_SWEEP_MAX_HIDDEN && (int64_t)hidden.size() == L &&
                  (int64_t)a.size() == L,
              op, ": need 1 .. ", NF_MADE_SWEEP_MAX_HIDDEN,
              " hidden layers plus the output layer, one h and one a per hidden layer");
  TORCH_CHECK(weights[0].dim() == 2 && q.dim() == 3, op,
              ": a hidden weight must be a matrix and q [B, D, P]");
  const int64_t B = gx.size(0), D = gx.size(1), H = weights[0].size(0), P = q.size(2);
  TORCH_CHECK(B >= 1 && B < (int64_t(1) << 31) && D >= 1 && H >= 1 && D < (1 << 24) &&
                  H < (1 << 24) && P >= 1 && P <= NF_SWEEP_ADJOINT_MAX_P,
              op, ": bad sizes B = ", B, ", D = ", D, ", H = ", H, ", P = ", P);
  TORCH_CHECK(nf_sweep_adjoint_rows((int)D, (int)H, (int)L, (int)P) > 0, op, ": (D, H, L, P) = (",
              D, ", ", H, ", ", L, ", ", P,
              ") exceeds the kernel's LDS budget (sweep_adjoint_supported)");
  const auto dev = gx.device();
  NfSweepAdjoint s{};
  s.B = (int)B; s.D = (int)D; s.H = (int)H; s.L = (int)L; s.P = (int)P;
  s.ldg = mat_stride(op, gx, "gx", B, D, dev);
  s.gx = gx.data_ptr<float>();
  s.ldd = mat_stride(op, d, "d", B, D, dev);
  s.d = d.data_ptr<float>();
  chk_vec(op, q, "q", B * D * P, at::kFloat, dev);
  chk_vec(op, c, "c", B * D * P, at::kFloat, dev);
  chk_vec(op, pbar, "pbar", B * D * P, at::kFloat, dev);
  s.q = q.data_ptr<float>();
  s.c = c.data_ptr<float>();
  s.pbar = pbar.data_ptr<float>();
  for (int64_t l = 0; l < L; ++l) {
    s.ldw[l] = mat_stride(op, weights[l], "a hidden weight", H, l == 0 ? D : H, dev);
    s.W[l] = weights[l].data_ptr<float>();
    s.ldh[l] = mat_stride(op, hidden[l], "a hidden activation", B, H, dev);
    s.h[l] = hidden[l].data_ptr<float>();
    s.lda[l] = mat_stride(op, a[l], "a hidden cotangent", B, H, dev);
    s.a[l] = a[l].data_ptr<float>();
  }
  s.ldo = mat_stride(op, weights[L], "the output weight", P * D, H, dev);
  s.Wo = weights[L].data_ptr<float>();
  chk_vec(op, perm, "perm", D, at::kInt, dev);
  chk_vec(op, ubeg, "ubeg", L * (D + 2), at::kInt, dev);
  s.perm = perm.data_ptr<int>();
  s.ubeg = ubeg.data_ptr<int>();
  s.ldwo = mat_stride(op, w, "w", B, D, dev);
  s.w = w.data_ptr<float>();
  nf_launch_sweep_adjoint(s, cur_stream());
}

// rows per block for (D, H, L, P); 0 when the shape does not fit or P is out of range
int64_t sweep_adjoint_rows(int64_t D, int64_t H, int64_t L, int64_t P) {
  if (D < 1 || H < 1 || L < 1 || D >= (1 << 24) || H >= (1 << 24) ||
      L > NF_MADE_SWEEP_MAX_HIDDEN || P < 1 || P > NF_SWEEP_ADJOINT_MAX_P)
    return 0;
  return nf_sweep_adjoint_rows((int)D, (int)H, (int)L, (int)P);
}

bool sweep_adjoint_supported(int64_t D, int64_t H, int64_t L, int64_t P) {
  return sweep_adjoint_rows(D, H, L, P) > 0;
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(vinf, m) {
  m.def("sweep_adjoint(Tensor gx, Tensor d, Tensor q, Tensor c, Tensor[] hidden, "
        "Tensor[] weights, Tensor perm, Tensor ubeg, Tensor(a!) w, Tensor(b!) pbar, "
        "Tensor(c!)[] a) -> ()");
  m.def("sweep_adjoint_rows(int D, int H, int L, int P) -> int", &sweep_adjoint_rows);
  m.def("sweep_adjoint_supported(int D, int H, int L, int P) -> bool", &sweep_adjoint_supported);
  m.def("made_sweep(Tensor v, Tensor[] weights, Tensor[] biases, Tensor perm, Tensor ubeg, "
        "int kind, float param, Tensor? ctx_bias, Tensor(a!) x, Tensor(b!) ldj) -> ()");
  m.def("made_sweep_rows(int D, int H, int L) -> int", &made_sweep_rows);
  m.def("made_sweep_supported(int D, int H, int L) -> bool", &made_sweep_supported);
  m.def("dsf_sweep(Tensor y, Tensor[] weights, Tensor[] biases, Tensor perm, Tensor ubeg, "
        "int units, Tensor? ctx_bias, Tensor(a!) x, Tensor(b!) ldj) -> ()");
  m.def("dsf_sweep_rows(int D, int H, int L, int U) -> int", &dsf_sweep_rows);
  m.def("dsf_sweep_supported(int D, int H, int L, int U) -> bool", &dsf_sweep_supported);
  m.def("rqs_sweep(Tensor y, Tensor[] weights, Tensor[] biases, Tensor perm, Tensor ubeg, "
        "int bins, float bound, Tensor? ctx_bias, Tensor(a!) x, Tensor(b!) ldj) -> ()");
  m.def("rqs_sweep_rows(int D, int H, int L, int K) -> int", &rqs_sweep_rows);
  m.def("rqs_sweep_supported(int D, int H, int L, int K) -> bool", &rqs_sweep_supported);
}

TORCH_LIBRARY_IMPL(vinf, CUDA, m) {
  m.impl("made_sweep", &made_sweep);
  m.impl("dsf_sweep", &dsf_sweep);
  m.impl("rqs_sweep", &rqs_sweep);
  m.impl("sweep_adjoint", &sweep_adjoint);
}
