// TORCH_LIBRARY fragment for the rational-quadratic spline coupling transform (spline.hip).
#include <torch/library.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include "launchers.h"

namespace {

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void chk_f32(const at::Tensor& t, const char* n) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous(), "rqs: ", n,
              " must be a contiguous fp32 GPU tensor");
}

void chk_params(const at::Tensor& p, const char* n) {
  TORCH_CHECK(p.is_cuda() && p.is_contiguous() &&
                  (p.scalar_type() == at::kFloat || p.scalar_type() == at::kBFloat16),
              "rqs: ", n, " must be a contiguous fp32 or bf16 GPU tensor");
}

// Shared shape checks; returns Dh.
int64_t chk_shapes(const at::Tensor& params, const at::Tensor& x, int64_t K, double bound) {
  TORCH_CHECK(K >= 2 && K <= 32, "rqs: need 2 <= K <= 32, got ", K);
  TORCH_CHECK(bound > 0, "rqs: need bound > 0, got ", bound);
  TORCH_CHECK(params.dim() == 2 && x.dim() == 2 && params.size(0) == x.size(0),
              "rqs: params [B, (3K-1) Dh] and x [B, Dh] expected");
  TORCH_CHECK(x.size(1) >= 1, "rqs: need Dh >= 1");
  TORCH_CHECK(params.size(1) == (3 * K - 1) * x.size(1), "rqs: params has ", params.size(1),
              " columns, expected (3K-1) Dh = ", (3 * K - 1) * x.size(1));
  TORCH_CHECK(params.device() == x.device(), "rqs: params and x on different devices");
  TORCH_CHECK(params.size(1) < (int64_t(1) << 29) && x.size(0) < (int64_t(1) << 31),
              "rqs: need (3K-1) Dh < 2^29 and B < 2^31");
  return x.size(1);
}

void rqs_fwd(const at::Tensor& params, const at::Tensor& x, int64_t K, double bound, bool inverse,
             bool ldj_init, const at::Tensor& y, const at::Tensor& ldj) {
  chk_params(params, "params");
  chk_f32(x, "x");
  chk_f32(y, "y");
  chk_f32(ldj, "ldj");
  const int64_t Dh = chk_shapes(params, x, K, bound);
  const int64_t B = x.size(0);
  TORCH_CHECK(y.sizes() == x.sizes() && ldj.numel() == B, "rqs: y [B, Dh] and ldj [B] expected");
  nf_launch_rqs_fwd(params.data_ptr(), params.scalar_type() == at::kBFloat16,
                    x.data_ptr<float>(), y.data_ptr<float>(), ldj.data_ptr<float>(), (int)B,
                    (int)Dh, (int)K, (float)bound, inverse, ldj_init, cur_stream());
}

void rqs_bwd(const at::Tensor& params, const at::Tensor& x, const at::Tensor& g_out,
             const at::Tensor& g_ldj, int64_t K, double bound, bool inverse,
             const at::Tensor& dparams, const at::Tensor& gx) {
  chk_params(params, "params");
  chk_params(dparams, "dparams");
  chk_f32(x, "x");
  chk_f32(g_out, "g_out");
  chk_f32(g_ldj, "g_ldj");
  chk_f32(gx, "gx");
  const int64_t Dh = chk_shapes(params, x, K, bound);
  const int64_t B = x.size(0);
  TORCH_CHECK(dparams.scalar_type() == params.scalar_type() && dparams.sizes() == params.sizes(),
              "rqs: dparams must match params in dtype and shape");
  TORCH_CHECK(g_out.sizes() == x.sizes() && gx.sizes() == x.sizes() && g_ldj.numel() == B,
              "rqs: g_out / gx [B, Dh] and g_ldj [B] expected");
  nf_launch_rqs_bwd(params.data_ptr(), params.scalar_type() == at::kBFloat16,
                    x.data_ptr<float>(), g_out.data_ptr<float>(), g_ldj.data_ptr<float>(),
                    dparams.data_ptr(), gx.data_ptr<float>(), (int)B, (int)Dh, (int)K,
                    (float)bound, inverse, cur_stream());
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(vinf, m) {
  m.def("rqs_fwd(Tensor params, Tensor x, int K, float bound, bool inverse, bool ldj_init, "
        "Tensor(a!) y, Tensor(b!) ldj) -> ()");
  m.def("rqs_bwd(Tensor params, Tensor x, Tensor g_out, Tensor g_ldj, int K, float bound, "
        "bool inverse, Tensor(a!) dparams, Tensor(b!) gx) -> ()");
}

TORCH_LIBRARY_IMPL(vinf, CUDA, m) {
  m.impl("rqs_fwd", &rqs_fwd);
  m.impl("rqs_bwd", &rqs_bwd);
}
