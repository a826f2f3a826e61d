// TORCH_LIBRARY fragment for the HMC trajectory kernel (glm_hmc.hip): L leapfrog steps and the
// accept step of B chains on a GLM posterior in one launch. Not differentiable; ops/hmc.py is the
// Python side.
#include <torch/library.h>
#include <ATen/ATen.h>

#include <cmath>

#include "bind_common.h"
#include "launchers.h"

namespace {

constexpr int64_t kMaxDim = 64;
constexpr int64_t kMaxLeapfrog = 1024;
constexpr int64_t kMaxRows = int64_t(1) << 31;

// theta0 / X: fp32 GPU [R, D], unit inner stride, any non-negative row stride
long row_stride(const at::Tensor& t, const char* n, int64_t D, const at::Device& dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev, "glm_hmc: ", n,
              " must be on the device of theta0");
  TORCH_CHECK(t.scalar_type() == at::kFloat, "glm_hmc: ", n, " must be fp32, got ",
              t.scalar_type());
  TORCH_CHECK(t.dim() == 2 && t.size(1) == D, "glm_hmc: ", n, " has shape ", t.sizes(),
              ", expected [rows, ", D, "]");
  TORCH_CHECK(t.size(0) >= 1 && t.size(0) < kMaxRows, "glm_hmc: ", n,
              " needs 1 <= rows < 2^31, got ", t.size(0));
  TORCH_CHECK(D == 1 || t.stride(1) == 1, "glm_hmc: ", n, " must have unit inner stride, got ",
              t.stride(1), " (only the row stride is free)");
  const int64_t rs = t.size(0) > 1 ? t.stride(0) : D;
  TORCH_CHECK(rs >= 0, "glm_hmc: ", n, " has a negative row stride");
  return (long)rs;
}

// a dense fp32 tensor of exactly this shape on the device of theta0
void chk_dense(const at::Tensor& t, const char* n, at::IntArrayRef shape, const at::Device& dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev && t.scalar_type() == at::kFloat,
              "glm_hmc: ", n, " must be an fp32 tensor on the device of theta0");
  TORCH_CHECK(t.sizes() == shape && t.is_contiguous(), "glm_hmc: ", n, " has shape ", t.sizes(),
              t.is_contiguous() ? "" : " (not contiguous)", ", expected a contiguous ", shape);
}

int chk_rows(const char* who, int64_t B, int64_t D, int64_t rows) {
  const int r = (rows >= 0 && rows <= 1024) ? nf_glm_hmc_rows((int)B, (int)D, (int)rows) : -1;
  TORCH_CHECK(r > 0, who, ": rows must be 0 (the launcher's choice) or one of the built tiles 32, "
              "64, 128, got ", rows);
  return r;
}

void glm_hmc_trajectory(const at::Tensor& theta0, const at::Tensor& p0, const at::Tensor& logp0,
                        const at::Tensor& grad0, const at::Tensor& eps,
                        const c10::optional<at::Tensor>& minv, const at::Tensor& log_u, int64_t L,
                        const at::Tensor& X, const at::Tensor& y,
                        const c10::optional<at::Tensor>& prec_dev, double prec_host,
                        bool has_prior, int64_t family, double inv_var, double scale, int64_t rows,
                        const at::Tensor& theta_prop, const at::Tensor& p_prop,
                        const at::Tensor& theta_out, const at::Tensor& logp_out,
                        const at::Tensor& grad_out, const at::Tensor& accept,
                        const at::Tensor& dH) {
  TORCH_CHECK(theta0.is_cuda(), "glm_hmc: theta0 must be a GPU tensor");
  TORCH_CHECK(theta0.dim() == 2, "glm_hmc: theta0 [B, D] expected, got ", theta0.dim(),
              " dimensions");
  const int64_t B = theta0.size(0), D = theta0.size(1);
  TORCH_CHECK(D >= 1 && D <= kMaxDim, "glm_hmc: need 1 <= D <= ", kMaxDim, ", got ", D);
  TORCH_CHECK(L >= 1 && L <= kMaxLeapfrog, "glm_hmc: need 1 <= L <= ", kMaxLeapfrog, ", got ", L);
  const auto dev = theta0.device();
  const long ldt = row_stride(theta0, "theta0", D, dev);
  const long ldx = row_stride(X, "X", D, dev);
  const int64_t N = X.size(0);
  TORCH_CHECK(y.is_cuda() && y.device() == dev, "glm_hmc: y must be on the device of theta0");
  TORCH_CHECK(y.scalar_type() == at::kFloat, "glm_hmc: y must be fp32, got ", y.scalar_type());
  TORCH_CHECK(y.dim() == 1 && y.size(0) == N && y.is_contiguous(), "glm_hmc: y has shape ",
              y.sizes(), ", expected a contiguous [", N, "] (one entry per row of X)");
  TORCH_CHECK(family >= 0 && family <= 2, "glm_hmc: unknown family ", family,
              " (0 = bernoulli, 1 = poisson, 2 = gaussian)");
  TORCH_CHECK(std::isfinite(inv_var) && inv_var > 0.0, "glm_hmc: inv_var must be positive, got ",
              inv_var);
  TORCH_CHECK(std::isfinite(scale) && scale > 0.0, "glm_hmc: scale must be positive, got ", scale);
  const float* pd = nullptr;
  if (has_prior) {
    if (prec_dev.has_value() && prec_dev->defined()) {
      chk_dense(*prec_dev, "prec_dev", {D}, dev);
      pd = prec_dev->data_ptr<float>();
    } else {
      TORCH_CHECK(std::isfinite(prec_host) && prec_host >= 0.0,
                  "glm_hmc: the prior precision must be >= 0, got prec_host = ", prec_host);
    }
  }
  const float* mi = nullptr;
  if (minv.has_value() && minv->defined()) {
    chk_dense(*minv, "minv", {D}, dev);
    mi = minv->data_ptr<float>();
  }
  chk_dense(p0, "p0", {B, D}, dev);
  chk_dense(grad0, "grad0", {B, D}, dev);
  chk_dense(logp0, "logp0", {B}, dev);
  chk_dense(eps, "eps", {B}, dev);
  chk_dense(log_u, "log_u", {B}, dev);
  chk_dense(theta_prop, "theta_prop", {B, D}, dev);
  chk_dense(p_prop, "p_prop", {B, D}, dev);
  chk_dense(theta_out, "theta_out", {B, D}, dev);
  chk_dense(grad_out, "grad_out", {B, D}, dev);
  chk_dense(logp_out, "logp_out", {B}, dev);
  chk_dense(accept, "accept", {B}, dev);
  chk_dense(dH, "dH", {B}, dev);
  // the kernel reads the inputs of a chain again when it rejects
  for (const at::Tensor* o : {&theta_prop, &p_prop, &theta_out, &grad_out, &logp_out})
    for (const at::Tensor* in : {&theta0, &p0, &grad0, &logp0})
      TORCH_CHECK(!o->is_alias_of(*in), "glm_hmc: an output shares storage with an input");
  const int r = chk_rows("glm_hmc", B, D, rows);
  nf_launch_glm_hmc_trajectory(
      theta0.data_ptr<float>(), ldt, p0.data_ptr<float>(), logp0.data_ptr<float>(),
      grad0.data_ptr<float>(), eps.data_ptr<float>(), mi, log_u.data_ptr<float>(), (int)L,
      X.data_ptr<float>(), ldx, y.data_ptr<float>(), pd, (float)prec_host, has_prior ? 1 : 0,
      (int)family, (float)inv_var, (float)scale, r, theta_prop.data_ptr<float>(),
      p_prop.data_ptr<float>(), theta_out.data_ptr<float>(), logp_out.data_ptr<float>(),
      grad_out.data_ptr<float>(), accept.data_ptr<float>(), dH.data_ptr<float>(), (int)B, (int)N,
      (int)D, cur_stream());
}

// chains per workgroup for (B, D); rows = 0 asks for the launcher's choice
int64_t glm_hmc_rows(int64_t B, int64_t D, int64_t rows) {
  TORCH_CHECK(B >= 1 && B < kMaxRows && D >= 1 && D <= kMaxDim,
              "glm_hmc_rows: need 1 <= B < 2^31 and 1 <= D <= ", kMaxDim);
  return chk_rows("glm_hmc_rows", B, D, rows);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(vinf, m) {
  m.def("glm_hmc_trajectory(Tensor theta0, Tensor p0, Tensor logp0, Tensor grad0, Tensor eps, "
        "Tensor? minv, Tensor log_u, int L, Tensor X, Tensor y, Tensor? prec_dev, "
        "float prec_host, bool has_prior, int family, float inv_var, float scale, int rows, "
        "Tensor(a!) theta_prop, Tensor(b!) p_prop, Tensor(c!) theta_out, Tensor(d!) logp_out, "
        "Tensor(e!) grad_out, Tensor(f!) accept, Tensor(g!) dH) -> ()");
  m.def("glm_hmc_rows(int B, int D, int rows) -> int", &glm_hmc_rows);
}

TORCH_LIBRARY_IMPL(vinf, CUDA, m) {
  m.impl("glm_hmc_trajectory", &glm_hmc_trajectory);
}
