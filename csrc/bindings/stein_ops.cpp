// TORCH_LIBRARY fragment for the all-pairs Stein kernels (stein.hip): SVGD direction and the
// row sums of the Stein kernel matrix. Neither op is differentiable.
#include <torch/library.h>
#include <ATen/ATen.h>

#include "bind_common.h"
#include "launchers.h"

namespace {

constexpr int64_t kMaxDim = 64;
constexpr int64_t kMaxSplits = 65535;   // gridDim.y

struct Problem {
  int64_t N, D;
  long ldx, lds;
  const float* h_dev;
  int S;
};

// x / score: fp32 GPU [N, D], unit inner stride, any non-negative row stride
long row_stride(const at::Tensor& t, const char* n, int64_t N, int64_t D, const at::Device& dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev, "stein: ", n, " must be on the device of x");
  TORCH_CHECK(t.scalar_type() == at::kFloat, "stein: ", n, " must be fp32, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 2 && t.size(0) == N && t.size(1) == D, "stein: ", n, " has shape ",
              t.sizes(), ", expected [", N, ", ", D, "]");
  TORCH_CHECK(D == 1 || t.stride(1) == 1, "stein: ", n, " must have unit inner stride, got ",
              t.stride(1), " (only the row stride is free)");
  const int64_t rs = N > 1 ? t.stride(0) : D;
  TORCH_CHECK(rs >= 0, "stein: ", n, " has a negative row stride");
  return (long)rs;
}

void chk_out(const at::Tensor& t, const char* n, int64_t numel, bool exact, const at::Device& dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev && t.scalar_type() == at::kFloat &&
                  t.is_contiguous(),
              "stein: ", n, " must be a contiguous fp32 tensor on the device of x");
  TORCH_CHECK(exact ? t.numel() == numel : t.numel() >= numel, "stein: ", n, " has ", t.numel(),
              " elements, need ", exact ? "" : "at least ", numel);
}

Problem chk_problem(const at::Tensor& x, const at::Tensor& score,
                    const c10::optional<at::Tensor>& h_dev, double h_host, int64_t kind,
                    int64_t j_splits) {
  TORCH_CHECK(x.is_cuda(), "stein: x must be a GPU tensor");
  TORCH_CHECK(x.dim() == 2, "stein: x [N, D] expected, got ", x.dim(), " dimensions");
  Problem p;
  p.N = x.size(0);
  p.D = x.size(1);
  TORCH_CHECK(p.D >= 1 && p.D <= kMaxDim, "stein: need 1 <= D <= ", kMaxDim, ", got ", p.D);
  TORCH_CHECK(p.N >= 1 && p.N < (int64_t(1) << 31), "stein: need 1 <= N < 2^31, got ", p.N);
  TORCH_CHECK(kind == 0 || kind == 1, "stein: unknown kind ", kind, " (0 = rbf, 1 = imq)");
  TORCH_CHECK(j_splits >= 0 && j_splits <= kMaxSplits, "stein: need 0 <= j_splits <= ",
              kMaxSplits, ", got ", j_splits);
  const auto dev = x.device();
  p.ldx = row_stride(x, "x", p.N, p.D, dev);
  p.lds = row_stride(score, "score", p.N, p.D, dev);
  p.h_dev = nullptr;
  if (h_dev.has_value() && h_dev->defined()) {
    const at::Tensor& h = *h_dev;
    TORCH_CHECK(h.is_cuda() && h.device() == dev && h.scalar_type() == at::kFloat &&
                    h.numel() == 1,
                "stein: h_dev must be a 1-element fp32 tensor on the device of x");
    p.h_dev = h.data_ptr<float>();
  } else {
    TORCH_CHECK(h_host > 0.0, "stein: the bandwidth must be positive, got h_host = ", h_host);
  }
  p.S = nf_stein_splits((int)p.N, (int)p.D, (int)j_splits);
  return p;
}

void stein_svgd(const at::Tensor& x, const at::Tensor& score,
                const c10::optional<at::Tensor>& h_dev, double h_host, int64_t kind,
                int64_t j_splits, const at::Tensor& phi, const at::Tensor& work) {
  const Problem p = chk_problem(x, score, h_dev, h_host, kind, j_splits);
  chk_out(phi, "phi", p.N * p.D, true, x.device());
  chk_out(work, "work", (int64_t)p.S * p.N * p.D, false, x.device());
  nf_launch_stein_svgd(x.data_ptr<float>(), p.ldx, score.data_ptr<float>(), p.lds, p.h_dev,
                       (float)h_host, (int)kind, p.S, phi.data_ptr<float>(),
                       work.data_ptr<float>(), (int)p.N, (int)p.D, cur_stream());
}

void stein_ksd_rows(const at::Tensor& x, const at::Tensor& score,
                    const c10::optional<at::Tensor>& h_dev, double h_host, int64_t kind,
                    int64_t j_splits, const at::Tensor& rows, const at::Tensor& diag,
                    const at::Tensor& work) {
  const Problem p = chk_problem(x, score, h_dev, h_host, kind, j_splits);
  chk_out(rows, "rows", p.N, true, x.device());
  chk_out(diag, "diag", p.N, true, x.device());
  chk_out(work, "work", (int64_t)p.S * p.N, false, x.device());
  nf_launch_stein_ksd(x.data_ptr<float>(), p.ldx, score.data_ptr<float>(), p.lds, p.h_dev,
                      (float)h_host, (int)kind, p.S, rows.data_ptr<float>(),
                      diag.data_ptr<float>(), work.data_ptr<float>(), (int)p.N, (int)p.D,
                      cur_stream());
}

// floats of workspace for mode 0 (svgd, [S, N, D]) or 1 (ksd, [S, N])
int64_t stein_workspace(int64_t N, int64_t D, int64_t j_splits, int64_t mode) {
  TORCH_CHECK(N >= 1 && N < (int64_t(1) << 31) && D >= 1 && D <= kMaxDim,
              "stein_workspace: need 1 <= N < 2^31 and 1 <= D <= ", kMaxDim);
  TORCH_CHECK(j_splits >= 0 && j_splits <= kMaxSplits, "stein_workspace: need 0 <= j_splits <= ",
              kMaxSplits, ", got ", j_splits);
  TORCH_CHECK(mode == 0 || mode == 1, "stein_workspace: mode 0 (svgd) or 1 (ksd), got ", mode);
  const int64_t S = nf_stein_splits((int)N, (int)D, (int)j_splits);
  return mode == 0 ? S * N * D : S * N;
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(vinf, m) {
  m.def("stein_svgd(Tensor x, Tensor score, Tensor? h_dev, float h_host, int kind, int j_splits, "
        "Tensor(a!) phi, Tensor(b!) work) -> ()");
  m.def("stein_ksd_rows(Tensor x, Tensor score, Tensor? h_dev, float h_host, int kind, "
        "int j_splits, Tensor(a!) rows, Tensor(b!) diag, Tensor(c!) work) -> ()");
  m.def("stein_workspace(int N, int D, int j_splits, int mode) -> int", &stein_workspace);
}

TORCH_LIBRARY_IMPL(vinf, CUDA, m) {
  m.impl("stein_svgd", &stein_svgd);
  m.impl("stein_ksd_rows", &stein_ksd_rows);
}
