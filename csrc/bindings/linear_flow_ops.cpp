// TORCH_LIBRARY fragment for the LU-linear flow and the full-rank Gaussian: the fused triangular
// solves of lu_solve.hip. The op itself is not differentiable; the gradient (one more launch with
// transpose = true plus fp32 weight-gradient products) is assembled in ops/linear_flow.py.
#include <torch/library.h>
#include <ATen/ATen.h>

#include "bind_common.h"
#include "launchers.h"

namespace {

// fp32 GPU [rows, cols] with unit inner stride; returns the row stride in elements
long lu_mat_stride(const at::Tensor& t, const char* n, int64_t rows, int64_t cols,
                   const at::Device& dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev, "lu_solve: ", n, " must be on the device of y");
  TORCH_CHECK(t.scalar_type() == at::kFloat, "lu_solve: ", n, " must be fp32, got ",
              t.scalar_type());
  TORCH_CHECK(t.dim() == 2 && t.size(0) == rows && t.size(1) == cols, "lu_solve: ", n,
              " has shape ", t.sizes(), ", expected [", rows, ", ", cols, "]");
  TORCH_CHECK(cols == 1 || t.stride(1) == 1, "lu_solve: ", n, " must have unit inner stride");
  const int64_t rs = rows > 1 ? t.stride(0) : cols;
  TORCH_CHECK(rs >= cols, "lu_solve: ", n, " has overlapping rows (row stride ", rs, ")");
  return (long)rs;
}

// y [B, D] -> x [B, D] (see launchers.h, NfLuSolve). A [D, D] is the packed factor, At = A^T its
// second orientation: transpose = false reads only At, transpose = true only A, and the one that
// is read must be given. mode 0 = LU, 1 = LOWER. check_perm = false skips the range check of perm
// (a device reduction and a host read) for a caller that has validated it; the kernel clamps.
void lu_solve(const at::Tensor& y, const c10::optional<at::Tensor>& A,
              const c10::optional<at::Tensor>& At, const c10::optional<at::Tensor>& perm,
              const c10::optional<at::Tensor>& bias, int64_t mode, bool transpose,
              bool check_perm, const at::Tensor& x) {
  TORCH_CHECK(y.is_cuda() && y.dim() == 2, "lu_solve: y must be a GPU tensor [B, D]");
  TORCH_CHECK(mode == 0 || mode == 1, "lu_solve: unknown mode ", mode, " (0 lu, 1 lower)");
  const int64_t B = y.size(0), D = y.size(1);
  TORCH_CHECK(B < (int64_t(1) << 31), "lu_solve: bad batch size ", B);
  TORCH_CHECK(D >= 1 && D < (1 << 24) && nf_lu_solve_rows((int)D) > 0, "lu_solve: D = ", D,
              " is outside the kernel's limits (lu_solve_supported)");
  const auto dev = y.device();
  const bool hasA = A.has_value() && A->defined(), hasAt = At.has_value() && At->defined();
  TORCH_CHECK(transpose ? hasA : hasAt, "lu_solve: transpose = ", transpose ? "true" : "false",
              " reads ", transpose ? "A" : "At = A^T", ", which was not given");
  NfLuSolve s{};
  s.B = (int)B; s.D = (int)D; s.mode = (int)mode; s.transpose = transpose ? 1 : 0;
  if (hasA) {
    const long ld = lu_mat_stride(*A, "A", D, D, dev);
    if (transpose) { s.M = A->data_ptr<float>(); s.ldm = ld; }
  }
  if (hasAt) {
    const long ld = lu_mat_stride(*At, "At", D, D, dev);
    if (!transpose) { s.M = At->data_ptr<float>(); s.ldm = ld; }
  }
  if (perm.has_value() && perm->defined()) {
    TORCH_CHECK(perm->is_cuda() && perm->device() == dev && perm->scalar_type() == at::kInt &&
                    perm->is_contiguous() && perm->numel() == D,
                "lu_solve: perm must be a contiguous int32 tensor of ", D,
                " elements on the device of y");
    if (check_perm)
      TORCH_CHECK(!at::logical_or(perm->lt(0), perm->ge(D)).any().item<bool>(),
                  "lu_solve: perm has entries outside [0, ", D, ")");
    s.perm = perm->data_ptr<int>();
  }
  if (bias.has_value() && bias->defined()) {
    TORCH_CHECK(bias->is_cuda() && bias->device() == dev && bias->scalar_type() == at::kFloat &&
                    bias->is_contiguous() && bias->numel() == D,
                "lu_solve: bias must be a contiguous fp32 tensor of ", D,
                " elements on the device of y");
    TORCH_CHECK(!transpose, "lu_solve: transpose = true takes no bias");
    s.bias = bias->data_ptr<float>();
  }
  if (B == 0) {
    TORCH_CHECK(x.is_cuda() && x.device() == dev && x.scalar_type() == at::kFloat &&
                    x.dim() == 2 && x.size(0) == 0 && x.size(1) == D,
                "lu_solve: x must be an fp32 [0, ", D, "] tensor on the device of y");
    return;
  }
  s.ldy = lu_mat_stride(y, "y", B, D, dev);
  s.y = y.data_ptr<float>();
  s.ldx = lu_mat_stride(x, "x", B, D, dev);
  s.x = x.data_ptr<float>();
  nf_launch_lu_solve(s, cur_stream());
}

// rows per block for D; 0 when D is not supported
int64_t lu_solve_rows(int64_t D) {
  if (D < 1 || D >= (1 << 24)) return 0;
  return nf_lu_solve_rows((int)D);
}

bool lu_solve_supported(int64_t D) { return lu_solve_rows(D) > 0; }

}  // namespace

TORCH_LIBRARY_FRAGMENT(vinf, m) {
  m.def("lu_solve(Tensor y, Tensor? A, Tensor? At, Tensor? perm, Tensor? bias, int mode, "
        "bool transpose, bool check_perm, Tensor(a!) x) -> ()");
  m.def("lu_solve_rows(int D) -> int", &lu_solve_rows);
  m.def("lu_solve_supported(int D) -> bool", &lu_solve_supported);
}

TORCH_LIBRARY_IMPL(vinf, CUDA, m) {
  m.impl("lu_solve", &lu_solve);
}
