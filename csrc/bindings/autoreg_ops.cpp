// TORCH_LIBRARY fragment for the autoregressive degree sweep (made_sweep.hip): MAF sampling and
// the IAF inverse in one masked pass. Not differentiable.
#include <torch/library.h>
#include <ATen/ATen.h>

#include "bind_common.h"
#include "launchers.h"

namespace {

// fp32 GPU [rows, cols] with unit inner stride; returns the row stride in elements
long mat_stride(const at::Tensor& t, const char* n, int64_t rows, int64_t cols,
                const at::Device& dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev, "made_sweep: ", n, " must be on the device of v");
  TORCH_CHECK(t.scalar_type() == at::kFloat, "made_sweep: ", n, " must be fp32, got ",
              t.scalar_type());
  TORCH_CHECK(t.dim() == 2 && t.size(0) == rows && t.size(1) == cols, "made_sweep: ", n,
              " has shape ", t.sizes(), ", expected [", rows, ", ", cols, "]");
  TORCH_CHECK(cols == 1 || t.stride(1) == 1, "made_sweep: ", n, " must have unit inner stride");
  const int64_t rs = rows > 1 ? t.stride(0) : cols;
  TORCH_CHECK(rs >= cols, "made_sweep: ", n, " has overlapping rows (row stride ", rs, ")");
  return (long)rs;
}

void chk_vec(const at::Tensor& t, const char* n, int64_t numel, at::ScalarType st,
             const at::Device& dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev && t.scalar_type() == st && t.is_contiguous() &&
                  t.numel() == numel,
              "made_sweep: ", n, " must be a contiguous ", st, " tensor of ", numel,
              " elements on the device of v");
}

void made_sweep(const at::Tensor& v, at::TensorList weights, at::TensorList biases,
                const at::Tensor& perm, const at::Tensor& ubeg, int64_t kind, double param,
                const c10::optional<at::Tensor>& ctx_bias, const at::Tensor& x,
                const at::Tensor& ldj) {
  TORCH_CHECK(v.is_cuda() && v.dim() == 2, "made_sweep: v must be a GPU tensor [B, D]");
  TORCH_CHECK(kind >= 0 && kind <= 2,
              "made_sweep: unknown kind ", kind, " (0 maf_sample, 1 iaf_gated, 2 iaf_affine)");
  const int64_t L = (int64_t)weights.size() - 1;
  TORCH_CHECK(L >= 1 && L <= NF_MADE_SWEEP_MAX_HIDDEN && biases.size() == weights.size(),
              "made_sweep: need 1 .. ", NF_MADE_SWEEP_MAX_HIDDEN,
              " hidden layers plus the output layer, one bias per weight");
  const int64_t B = v.size(0), D = v.size(1), H = weights[0].size(0);
  TORCH_CHECK(B >= 1 && B < (int64_t(1) << 31) && D >= 1 && H >= 1 && D < (1 << 24) &&
                  H < (1 << 24),
              "made_sweep: bad sizes B = ", B, ", D = ", D, ", H = ", H);
  TORCH_CHECK(nf_made_sweep_rows((int)D, (int)H, (int)L) > 0, "made_sweep: (D, H, L) = (", D, ", ",
              H, ", ", L, ") exceeds the kernel's LDS budget (made_sweep_supported)");
  const auto dev = v.device();
  NfMadeSweep s{};
  s.B = (int)B; s.D = (int)D; s.H = (int)H; s.L = (int)L; s.kind = (int)kind;
  s.param = (float)param;
  s.ldv = mat_stride(v, "v", B, D, dev);
  s.v = v.data_ptr<float>();
  for (int64_t l = 0; l < L; ++l) {
    s.ldw[l] = mat_stride(weights[l], "a hidden weight", H, l == 0 ? D : H, dev);
    s.W[l] = weights[l].data_ptr<float>();
    chk_vec(biases[l], "a hidden bias", H, at::kFloat, dev);
    s.b[l] = biases[l].data_ptr<float>();
  }
  s.ldo = mat_stride(weights[L], "the output weight", 2 * D, H, dev);
  s.Wo = weights[L].data_ptr<float>();
  chk_vec(biases[L], "the output bias", 2 * D, at::kFloat, dev);
  s.bo = biases[L].data_ptr<float>();
  chk_vec(perm, "perm", D, at::kInt, dev);
  chk_vec(ubeg, "ubeg", L * (D + 2), at::kInt, dev);
  s.perm = perm.data_ptr<int>();
  s.ubeg = ubeg.data_ptr<int>();
  if (ctx_bias.has_value() && ctx_bias->defined()) {
    s.ldc = mat_stride(*ctx_bias, "ctx_bias", B, H, dev);
    s.ctx = ctx_bias->data_ptr<float>();
  }
  s.ldx = mat_stride(x, "x", B, D, dev);
  s.x = x.data_ptr<float>();
  chk_vec(ldj, "ldj", B, at::kFloat, dev);
  s.ldj = ldj.data_ptr<float>();
  nf_launch_made_sweep(s, cur_stream());
}

// rows per block for (D, H, L); 0 when the shape does not fit
int64_t made_sweep_rows(int64_t D, int64_t H, int64_t L) {
  if (D < 1 || H < 1 || L < 1 || D >= (1 << 24) || H >= (1 << 24) || L > NF_MADE_SWEEP_MAX_HIDDEN)
    return 0;
  return nf_made_sweep_rows((int)D, (int)H, (int)L);
}

bool made_sweep_supported(int64_t D, int64_t H, int64_t L) { return made_sweep_rows(D, H, L) > 0; }

}  // namespace

TORCH_LIBRARY_FRAGMENT(vinf, m) {
  m.def("made_sweep(Tensor v, Tensor[] weights, Tensor[] biases, Tensor perm, Tensor ubeg, "
        "int kind, float param, Tensor? ctx_bias, Tensor(a!) x, Tensor(b!) ldj) -> ()");
  m.def("made_sweep_rows(int D, int H, int L) -> int", &made_sweep_rows);
  m.def("made_sweep_supported(int D, int H, int L) -> bool", &made_sweep_supported);
}

TORCH_LIBRARY_IMPL(vinf, CUDA, m) {
  m.impl("made_sweep", &made_sweep);
}
