// TORCH_LIBRARY fragment for the element-wise flow transforms: the rational-quadratic spline
// (spline.hip) and the deep sigmoidal flow (dsf.hip). Both take plane-major params
// [B, planes D] (fp32 or bf16) and x [B, D], so one set of checks serves the four ops.
#include <torch/library.h>
#include <ATen/ATen.h>

#include "bind_common.h"
#include "launchers.h"

namespace {

// One call's transform: message tag, the per-element count (n bins or units, by name, with its
// lower limit) and the planes per element that follow from it.
struct Flow {
  const char* tag;
  const char* count;
  int64_t n_min, n, planes;
};

Flow rqs(int64_t K) { return {"rqs", "K", 2, K, 3 * K - 1}; }
Flow dsf(int64_t H) { return {"dsf", "H", 1, H, 3 * H}; }

void chk_f32(const Flow& f, const at::Tensor& t, const char* n) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous(), f.tag, ": ", n,
              " must be a contiguous fp32 GPU tensor");
}

void chk_params(const Flow& f, const at::Tensor& p, const char* n) {
  TORCH_CHECK(p.is_cuda() && p.is_contiguous() &&
                  (p.scalar_type() == at::kFloat || p.scalar_type() == at::kBFloat16),
              f.tag, ": ", n, " must be a contiguous fp32 or bf16 GPU tensor");
}

// params [B, planes D], x and every tensor of like_x [B, D], rows [B] (ldj or g_ldj).
void chk_call(const Flow& f, const at::Tensor& params, const at::Tensor& x,
              std::initializer_list<std::pair<const char*, const at::Tensor*>> like_x,
              const char* rows_name, const at::Tensor& rows) {
  chk_params(f, params, "params");
  chk_f32(f, x, "x");
  for (const auto& t : like_x) chk_f32(f, *t.second, t.first);
  chk_f32(f, rows, rows_name);
  TORCH_CHECK(f.n >= f.n_min && f.n <= 32, f.tag, ": need ", f.n_min, " <= ", f.count,
              " <= 32, got ", f.n);
  TORCH_CHECK(params.dim() == 2 && x.dim() == 2, f.tag, ": params [B, planes D] and x [B, D] ",
              "expected");
  TORCH_CHECK(params.size(0) == x.size(0), f.tag, ": params has ", params.size(0),
              " rows, x has ", x.size(0));
  TORCH_CHECK(x.size(1) >= 1, f.tag, ": need D >= 1");
  TORCH_CHECK(params.size(1) == f.planes * x.size(1), f.tag, ": params has ", params.size(1),
              " columns, expected ", f.planes, " D = ", f.planes * x.size(1), " for ", f.count,
              " = ", f.n);
  TORCH_CHECK(params.device() == x.device(), f.tag, ": params and x on different devices");
  TORCH_CHECK(params.size(1) < (int64_t(1) << 29) && x.size(0) < (int64_t(1) << 31), f.tag,
              ": need planes D < 2^29 and B < 2^31");
  for (const auto& t : like_x)
    TORCH_CHECK(t.second->sizes() == x.sizes(), f.tag, ": ", t.first,
                " must have the shape of x");
  TORCH_CHECK(rows.numel() == x.size(0), f.tag, ": ", rows_name, " has ", rows.numel(),
              " rows, x has ", x.size(0));
}

void chk_fwd(const Flow& f, const at::Tensor& params, const at::Tensor& x, const at::Tensor& y,
             const at::Tensor& ldj) {
  chk_call(f, params, x, {{"y", &y}}, "ldj", ldj);
}

void chk_bwd(const Flow& f, const at::Tensor& params, const at::Tensor& x,
             const at::Tensor& g_out, const at::Tensor& g_ldj, const at::Tensor& dparams,
             const at::Tensor& gx) {
  chk_params(f, dparams, "dparams");
  chk_call(f, params, x, {{"g_out", &g_out}, {"gx", &gx}}, "g_ldj", g_ldj);
  TORCH_CHECK(dparams.scalar_type() == params.scalar_type() && dparams.sizes() == params.sizes(),
              f.tag, ": dparams must match params in dtype and shape");
}

void chk_bound(double bound) { TORCH_CHECK(bound > 0, "rqs: need bound > 0, got ", bound); }

bool is_bf16(const at::Tensor& t) { return t.scalar_type() == at::kBFloat16; }

void rqs_fwd(const at::Tensor& params, const at::Tensor& x, int64_t K, double bound, bool inverse,
             bool ldj_init, const at::Tensor& y, const at::Tensor& ldj) {
  chk_fwd(rqs(K), params, x, y, ldj);
  chk_bound(bound);
  nf_launch_rqs_fwd(params.data_ptr(), is_bf16(params), x.data_ptr<float>(), y.data_ptr<float>(),
                    ldj.data_ptr<float>(), (int)x.size(0), (int)x.size(1), (int)K, (float)bound,
                    inverse, ldj_init, cur_stream());
}

void rqs_bwd(const at::Tensor& params, const at::Tensor& x, const at::Tensor& g_out,
             const at::Tensor& g_ldj, int64_t K, double bound, bool inverse,
             const at::Tensor& dparams, const at::Tensor& gx) {
  chk_bwd(rqs(K), params, x, g_out, g_ldj, dparams, gx);
  chk_bound(bound);
  nf_launch_rqs_bwd(params.data_ptr(), is_bf16(params), x.data_ptr<float>(),
                    g_out.data_ptr<float>(), g_ldj.data_ptr<float>(), dparams.data_ptr(),
                    gx.data_ptr<float>(), (int)x.size(0), (int)x.size(1), (int)K, (float)bound,
                    inverse, cur_stream());
}

void dsf_fwd(const at::Tensor& params, const at::Tensor& x, int64_t H, bool inverse, bool init,
             const at::Tensor& y, const at::Tensor& ldj) {
  chk_fwd(dsf(H), params, x, y, ldj);
  nf_launch_dsf_fwd(params.data_ptr(), is_bf16(params), x.data_ptr<float>(), y.data_ptr<float>(),
                    ldj.data_ptr<float>(), (int)x.size(0), (int)x.size(1), (int)H, inverse, init,
                    cur_stream());
}

void dsf_bwd(const at::Tensor& params, const at::Tensor& x, const at::Tensor& g_out,
             const at::Tensor& g_ldj, int64_t H, bool inverse, const at::Tensor& dparams,
             const at::Tensor& gx) {
  chk_bwd(dsf(H), params, x, g_out, g_ldj, dparams, gx);
  nf_launch_dsf_bwd(params.data_ptr(), is_bf16(params), x.data_ptr<float>(),
                    g_out.data_ptr<float>(), g_ldj.data_ptr<float>(), dparams.data_ptr(),
                    gx.data_ptr<float>(), (int)x.size(0), (int)x.size(1), (int)H, inverse,
                    cur_stream());
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(vinf, m) {
  m.def("rqs_fwd(Tensor params, Tensor x, int K, float bound, bool inverse, bool ldj_init, "
        "Tensor(a!) y, Tensor(b!) ldj) -> ()");
  m.def("rqs_bwd(Tensor params, Tensor x, Tensor g_out, Tensor g_ldj, int K, float bound, "
        "bool inverse, Tensor(a!) dparams, Tensor(b!) gx) -> ()");
  m.def("dsf_fwd(Tensor params, Tensor x, int H, bool inverse, bool init, Tensor(a!) y, "
        "Tensor(b!) ldj) -> ()");
  m.def("dsf_bwd(Tensor params, Tensor x, Tensor g_out, Tensor g_ldj, int H, bool inverse, "
        "Tensor(a!) dparams, Tensor(b!) gx) -> ()");
}

TORCH_LIBRARY_IMPL(vinf, CUDA, m) {
  m.impl("rqs_fwd", &rqs_fwd);
  m.impl("rqs_bwd", &rqs_bwd);
  m.impl("dsf_fwd", &dsf_fwd);
  m.impl("dsf_bwd", &dsf_bwd);
}
