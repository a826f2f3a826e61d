// TORCH_LIBRARY fragment for the GLM likelihood kernel (glm.hip): log-density and score of B
// parameter rows against N data rows, and for the pass that adds the negative Hessian
// (glm_hess.hip). The ops are not differentiable; ops/glm.py wraps the first in an
// autograd.Function that hands the score back as the gradient.
#include <torch/library.h>
#include <ATen/ATen.h>

#include <cmath>

#include "bind_common.h"
#include "launchers.h"

namespace {

constexpr int64_t kMaxDim = 64;
constexpr int64_t kMaxSplits = 65535;   // gridDim.y
constexpr int64_t kMaxRows = int64_t(1) << 31;

// theta / X: fp32 GPU [R, D], unit inner stride, any non-negative row stride
long row_stride(const at::Tensor& t, const char* n, int64_t D, const at::Device& dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev, "glm: ", n, " must be on the device of theta");
  TORCH_CHECK(t.scalar_type() == at::kFloat, "glm: ", n, " must be fp32, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 2 && t.size(1) == D, "glm: ", n, " has shape ", t.sizes(),
              ", expected [rows, ", D, "]");
  TORCH_CHECK(t.size(0) >= 1 && t.size(0) < kMaxRows, "glm: ", n, " needs 1 <= rows < 2^31, got ",
              t.size(0));
  TORCH_CHECK(D == 1 || t.stride(1) == 1, "glm: ", n, " must have unit inner stride, got ",
              t.stride(1), " (only the row stride is free)");
  const int64_t rs = t.size(0) > 1 ? t.stride(0) : D;
  TORCH_CHECK(rs >= 0, "glm: ", n, " has a negative row stride");
  return (long)rs;
}

void chk_out(const at::Tensor& t, const char* n, int64_t numel, bool exact, const at::Device& dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev && t.scalar_type() == at::kFloat &&
                  t.is_contiguous(),
              "glm: ", n, " must be a contiguous fp32 tensor on the device of theta");
  TORCH_CHECK(exact ? t.numel() == numel : t.numel() >= numel, "glm: ", n, " has ", t.numel(),
              " elements, need ", exact ? "" : "at least ", numel);
}

void chk_splits(const char* who, int64_t n_splits) {
  TORCH_CHECK(n_splits >= 0 && n_splits <= kMaxSplits, who, ": need 0 <= n_splits <= ", kMaxSplits,
              ", got ", n_splits);
}

// the inputs of a pass, checked
struct GlmIn {
  int64_t B, N, D;
  long ldt, ldx;
  const float* prec_dev;
  at::Device dev;
};

GlmIn chk_inputs(const at::Tensor& theta, const at::Tensor& X, const at::Tensor& y,
                 const c10::optional<at::Tensor>& prec_dev, double prec_host, bool has_prior,
                 int64_t family, double inv_var, double scale, int64_t n_splits) {
  TORCH_CHECK(theta.is_cuda(), "glm: theta must be a GPU tensor");
  TORCH_CHECK(theta.dim() == 2, "glm: theta [B, D] expected, got ", theta.dim(), " dimensions");
  const int64_t B = theta.size(0), D = theta.size(1);
  TORCH_CHECK(D >= 1 && D <= kMaxDim, "glm: need 1 <= D <= ", kMaxDim, ", got ", D);
  const auto dev = theta.device();
  const long ldt = row_stride(theta, "theta", D, dev);
  const long ldx = row_stride(X, "X", D, dev);
  const int64_t N = X.size(0);
  TORCH_CHECK(y.is_cuda() && y.device() == dev, "glm: y must be on the device of theta");
  TORCH_CHECK(y.scalar_type() == at::kFloat, "glm: y must be fp32, got ", y.scalar_type());
  TORCH_CHECK(y.dim() == 1 && y.size(0) == N && y.is_contiguous(), "glm: y has shape ", y.sizes(),
              ", expected a contiguous [", N, "] (one entry per row of X)");
  TORCH_CHECK(family >= 0 && family <= 2, "glm: unknown family ", family,
              " (0 = bernoulli, 1 = poisson, 2 = gaussian)");
  TORCH_CHECK(std::isfinite(inv_var) && inv_var > 0.0, "glm: inv_var must be positive, got ",
              inv_var);
  TORCH_CHECK(std::isfinite(scale) && scale > 0.0, "glm: scale must be positive, got ", scale);
  chk_splits("glm", n_splits);
  const float* pd = nullptr;
  if (has_prior) {
    if (prec_dev.has_value() && prec_dev->defined()) {
      const at::Tensor& p = *prec_dev;
      TORCH_CHECK(p.is_cuda() && p.device() == dev && p.scalar_type() == at::kFloat &&
                      p.dim() == 1 && p.size(0) == D && p.is_contiguous(),
                  "glm: prec_dev must be a contiguous fp32 [", D, "] tensor on the device of theta");
      pd = p.data_ptr<float>();
    } else {
      TORCH_CHECK(std::isfinite(prec_host) && prec_host >= 0.0,
                  "glm: the prior precision must be >= 0, got prec_host = ", prec_host);
    }
  }
  return GlmIn{B, N, D, ldt, ldx, pd, dev};
}

void glm_logp_grad(const at::Tensor& theta, const at::Tensor& X, const at::Tensor& y,
                   const c10::optional<at::Tensor>& prec_dev, double prec_host, bool has_prior,
                   int64_t family, double inv_var, double scale, int64_t n_splits,
                   const at::Tensor& logp, const at::Tensor& grad, const at::Tensor& work) {
  const GlmIn in = chk_inputs(theta, X, y, prec_dev, prec_host, has_prior, family, inv_var, scale,
                              n_splits);
  const int64_t B = in.B, N = in.N, D = in.D;
  const int S = nf_glm_splits((int)B, (int)N, (int)D, (int)n_splits);
  chk_out(logp, "logp", B, true, in.dev);
  chk_out(grad, "grad", B * D, true, in.dev);
  chk_out(work, "work", (int64_t)S * B * (D + 1), false, in.dev);
  nf_launch_glm_logp_grad(theta.data_ptr<float>(), in.ldt, X.data_ptr<float>(), in.ldx,
                          y.data_ptr<float>(), in.prec_dev, (float)prec_host, has_prior ? 1 : 0,
                          (int)family, (float)inv_var, (float)scale, S, logp.data_ptr<float>(),
                          grad.data_ptr<float>(), work.data_ptr<float>(), (int)B, (int)N, (int)D,
                          cur_stream());
}

// logp, grad and hess [B, D, D] (the negative Hessian of logp) from one pass of glm_hess.hip
void glm_logp_grad_hess(const at::Tensor& theta, const at::Tensor& X, const at::Tensor& y,
                        const c10::optional<at::Tensor>& prec_dev, double prec_host,
                        bool has_prior, int64_t family, double inv_var, double scale,
                        int64_t n_splits, const at::Tensor& logp, const at::Tensor& grad,
                        const at::Tensor& hess, const at::Tensor& work) {
  const GlmIn in = chk_inputs(theta, X, y, prec_dev, prec_host, has_prior, family, inv_var, scale,
                              n_splits);
  const int64_t B = in.B, N = in.N, D = in.D;
  const int S = nf_glm_hess_splits((int)B, (int)N, (int)D, (int)n_splits);
  chk_out(logp, "logp", B, true, in.dev);
  chk_out(grad, "grad", B * D, true, in.dev);
  chk_out(hess, "hess", B * D * D, true, in.dev);
  chk_out(work, "work", (int64_t)S * B * (D * D + D + 1), false, in.dev);
  nf_launch_glm_logp_grad_hess(theta.data_ptr<float>(), in.ldt, X.data_ptr<float>(), in.ldx,
                               y.data_ptr<float>(), in.prec_dev, (float)prec_host,
                               has_prior ? 1 : 0, (int)family, (float)inv_var, (float)scale, S,
                               logp.data_ptr<float>(), grad.data_ptr<float>(),
                               hess.data_ptr<float>(), work.data_ptr<float>(), (int)B, (int)N,
                               (int)D, cur_stream());
}

// floats of workspace: [S, B, D + 1]
int64_t glm_workspace(int64_t B, int64_t N, int64_t D, int64_t n_splits) {
  TORCH_CHECK(B >= 1 && B < kMaxRows && N >= 1 && N < kMaxRows && D >= 1 && D <= kMaxDim,
              "glm_workspace: need 1 <= B, N < 2^31 and 1 <= D <= ", kMaxDim);
  chk_splits("glm_workspace", n_splits);
  return (int64_t)nf_glm_splits((int)B, (int)N, (int)D, (int)n_splits) * B * (D + 1);
}

// floats of workspace: [S, B, D D + D + 1]
int64_t glm_hess_workspace(int64_t B, int64_t N, int64_t D, int64_t n_splits) {
  TORCH_CHECK(B >= 1 && B < kMaxRows && N >= 1 && N < kMaxRows && D >= 1 && D <= kMaxDim,
              "glm_hess_workspace: need 1 <= B, N < 2^31 and 1 <= D <= ", kMaxDim);
  chk_splits("glm_hess_workspace", n_splits);
  return (int64_t)nf_glm_hess_splits((int)B, (int)N, (int)D, (int)n_splits) * B * (D * D + D + 1);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(vinf, m) {
  m.def("glm_logp_grad(Tensor theta, Tensor X, Tensor y, Tensor? prec_dev, float prec_host, "
        "bool has_prior, int family, float inv_var, float scale, int n_splits, "
        "Tensor(a!) logp, Tensor(b!) grad, Tensor(c!) work) -> ()");
  m.def("glm_workspace(int B, int N, int D, int n_splits) -> int", &glm_workspace);
  m.def("glm_logp_grad_hess(Tensor theta, Tensor X, Tensor y, Tensor? prec_dev, float prec_host, "
        "bool has_prior, int family, float inv_var, float scale, int n_splits, "
        "Tensor(a!) logp, Tensor(b!) grad, Tensor(c!) hess, Tensor(d!) work) -> ()");
  m.def("glm_hess_workspace(int B, int N, int D, int n_splits) -> int", &glm_hess_workspace);
}

TORCH_LIBRARY_IMPL(vinf, CUDA, m) {
  m.impl("glm_logp_grad", &glm_logp_grad);
  m.impl("glm_logp_grad_hess", &glm_logp_grad_hess);
}
