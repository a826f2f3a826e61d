// TORCH_LIBRARY fragment for the deep sigmoidal flow transformer (dsf.hip).
#include <torch/library.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include "launchers.h"

namespace {

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void chk_f32(const at::Tensor& t, const char* n) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous(), "dsf: ", n,
              " must be a contiguous fp32 GPU tensor");
}

void chk_params(const at::Tensor& p, const char* n) {
  TORCH_CHECK(p.is_cuda() && p.is_contiguous() &&
                  (p.scalar_type() == at::kFloat || p.scalar_type() == at::kBFloat16),
              "dsf: ", n, " must be a contiguous fp32 or bf16 GPU tensor");
}

// Shared shape checks; returns D.
int64_t chk_shapes(const at::Tensor& params, const at::Tensor& x, int64_t H) {
  TORCH_CHECK(H >= 1 && H <= 32, "dsf: need 1 <= H <= 32, got ", H);
  TORCH_CHECK(params.dim() == 2 && x.dim() == 2, "dsf: params [B, 3H D] and x [B, D] expected");
  TORCH_CHECK(params.size(0) == x.size(0), "dsf: params has ", params.size(0), " rows, x has ",
              x.size(0));
  TORCH_CHECK(x.size(1) >= 1, "dsf: need D >= 1");
  TORCH_CHECK(params.size(1) == 3 * H * x.size(1), "dsf: params has ", params.size(1),
              " columns, expected 3H D = ", 3 * H * x.size(1));
  TORCH_CHECK(params.device() == x.device(), "dsf: params and x on different devices");
  TORCH_CHECK(params.size(1) < (int64_t(1) << 29) && x.size(0) < (int64_t(1) << 31),
              "dsf: need 3H D < 2^29 and B < 2^31");
  return x.size(1);
}

void dsf_fwd(const at::Tensor& params, const at::Tensor& x, int64_t H, bool inverse, bool init,
             const at::Tensor& y, const at::Tensor& ldj) {
  chk_params(params, "params");
  chk_f32(x, "x");
  chk_f32(y, "y");
  chk_f32(ldj, "ldj");
  const int64_t D = chk_shapes(params, x, H);
  const int64_t B = x.size(0);
  TORCH_CHECK(y.sizes() == x.sizes(), "dsf: y must have the shape of x");
  TORCH_CHECK(ldj.numel() == B, "dsf: ldj has ", ldj.numel(), " rows, x has ", B);
  nf_launch_dsf_fwd(params.data_ptr(), params.scalar_type() == at::kBFloat16,
                    x.data_ptr<float>(), y.data_ptr<float>(), ldj.data_ptr<float>(), (int)B,
                    (int)D, (int)H, inverse, init, cur_stream());
}

void dsf_bwd(const at::Tensor& params, const at::Tensor& x, const at::Tensor& g_out,
             const at::Tensor& g_ldj, int64_t H, bool inverse, const at::Tensor& dparams,
             const at::Tensor& gx) {
  chk_params(params, "params");
  chk_params(dparams, "dparams");
  chk_f32(x, "x");
  chk_f32(g_out, "g_out");
  chk_f32(g_ldj, "g_ldj");
  chk_f32(gx, "gx");
  const int64_t D = chk_shapes(params, x, H);
  const int64_t B = x.size(0);
  TORCH_CHECK(dparams.scalar_type() == params.scalar_type() && dparams.sizes() == params.sizes(),
              "dsf: dparams must match params in dtype and shape");
  TORCH_CHECK(g_out.sizes() == x.sizes() && gx.sizes() == x.sizes(),
              "dsf: g_out and gx must have the shape of x");
  TORCH_CHECK(g_ldj.numel() == B, "dsf: g_ldj has ", g_ldj.numel(), " rows, x has ", B);
  nf_launch_dsf_bwd(params.data_ptr(), params.scalar_type() == at::kBFloat16,
                    x.data_ptr<float>(), g_out.data_ptr<float>(), g_ldj.data_ptr<float>(),
                    dparams.data_ptr(), gx.data_ptr<float>(), (int)B, (int)D, (int)H, inverse,
                    cur_stream());
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(vinf, m) {
  m.def("dsf_fwd(Tensor params, Tensor x, int H, bool inverse, bool init, Tensor(a!) y, "
        "Tensor(b!) ldj) -> ()");
  m.def("dsf_bwd(Tensor params, Tensor x, Tensor g_out, Tensor g_ldj, int H, bool inverse, "
        "Tensor(a!) dparams, Tensor(b!) gx) -> ()");
}

TORCH_LIBRARY_IMPL(vinf, CUDA, m) {
  m.impl("dsf_fwd", &dsf_fwd);
  m.impl("dsf_bwd", &dsf_bwd);
}
