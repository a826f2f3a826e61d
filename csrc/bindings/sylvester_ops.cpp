// TORCH_LIBRARY fragment for the fused Sylvester flow stack (sylvester.hip).
#include <torch/library.h>
#include <ATen/ATen.h>

#include <vector>

#include "bind_common.h"
#include "launchers.h"

namespace {

void chk_dense(const at::Tensor& t, const char* n, at::IntArrayRef sizes) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous(), "sylvester: ", n,
              " must be a contiguous fp32 GPU tensor");
  TORCH_CHECK(t.sizes() == sizes, "sylvester: ", n, " has shape ", t.sizes(), ", expected ", sizes);
}

struct RowView {
  float* p;
  long rs;
};

// t is [K, inner...] (shared, row stride 0; parameters only) or [N, K, inner...] with the
// [K, inner...] block of a row dense and any non-negative row stride.
RowView row_view(const at::Tensor& t, const char* n, int64_t N, int64_t K,
                 std::vector<int64_t> inner, bool is_output, const at::Device& dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev, "sylvester: ", n, " must be on the device of z");
  TORCH_CHECK(t.scalar_type() == at::kFloat, "sylvester: ", n, " must be fp32, got ",
              t.scalar_type());
  inner.insert(inner.begin(), K);
  const int64_t nd = (int64_t)inner.size();
  const bool per_row = t.dim() == nd + 1;
  TORCH_CHECK(per_row || (!is_output && t.dim() == nd), "sylvester: ", n, " has ", t.dim(),
              " dimensions, expected ", is_output ? "" : "[K, ...] or ", "[N, K, ...]");
  const int64_t off = per_row ? 1 : 0;
  TORCH_CHECK(!per_row || t.size(0) == N, "sylvester: ", n, " has ", t.size(0), " rows, z has ", N);
  int64_t expect = 1, block = 1;
  for (int64_t d = nd - 1; d >= 0; --d) block *= inner[d];
  for (int64_t d = nd - 1; d >= 0; --d) {
    TORCH_CHECK(t.size(off + d) == inner[d], "sylvester: ", n, " has shape ", t.sizes(),
                ", expected inner sizes ", at::IntArrayRef(inner),
                " (R packed strict-upper: D (D - 1) / 2 entries)");
    TORCH_CHECK(block == 0 || inner[d] == 1 || t.stride(off + d) == expect, "sylvester: ", n,
                " must have dense inner dimensions (only the row stride is free); strides ",
                t.strides());
    expect *= inner[d];
  }
  long rs = 0;
  if (per_row && N > 1) {
    rs = (long)t.stride(0);
    TORCH_CHECK(rs >= 0, "sylvester: ", n, " has a negative row stride");
    TORCH_CHECK(!is_output || rs >= block, "sylvester: rows of ", n, " overlap");
  }
  return RowView{block == 0 ? nullptr : t.data_ptr<float>(), rs};
}

struct Dims {
  int64_t N, D, K, H, P;
};

Dims chk_dims(const at::Tensor& z, const at::Tensor& V, at::IntArrayRef flips) {
  TORCH_CHECK(z.dim() == 2, "sylvester: z [N, D] expected");
  TORCH_CHECK(V.dim() == 3 || V.dim() == 4, "sylvester: V [K, H, D] or [N, K, H, D] expected");
  Dims s;
  s.N = z.size(0);
  s.D = z.size(1);
  s.K = V.size(V.dim() - 3);
  s.H = V.size(V.dim() - 2);
  s.P = s.D * (s.D - 1) / 2;
  TORCH_CHECK(s.D >= 1 && s.D <= 64, "sylvester: need 1 <= D <= 64, got ", s.D);
  TORCH_CHECK(s.H <= 16, "sylvester: need 0 <= H <= 16, got ", s.H);
  TORCH_CHECK(s.K >= 1, "sylvester: need K >= 1");
  TORCH_CHECK((int64_t)flips.size() == s.K, "sylvester: ", flips.size(), " flips for K = ", s.K,
              " layers");
  TORCH_CHECK(s.N < (int64_t(1) << 31), "sylvester: need N < 2^31, got ", s.N);
  TORCH_CHECK(s.K < (int64_t(1) << 31), "sylvester: need K < 2^31, got ", s.K);
  return s;
}

NfSylParams params_of(const Dims& s, const at::Tensor& z, const at::Tensor& R1,
                      const at::Tensor& R2, const at::Tensor& d1, const at::Tensor& d2,
                      const at::Tensor& b, const at::Tensor& V) {
  const auto dev = z.device();
  const RowView r1 = row_view(R1, "R1", s.N, s.K, {s.P}, false, dev);
  const RowView r2 = row_view(R2, "R2", s.N, s.K, {s.P}, false, dev);
  const RowView a1 = row_view(d1, "d1", s.N, s.K, {s.D}, false, dev);
  const RowView a2 = row_view(d2, "d2", s.N, s.K, {s.D}, false, dev);
  const RowView bb = row_view(b, "b", s.N, s.K, {s.D}, false, dev);
  const RowView vv = row_view(V, "V", s.N, s.K, {s.H, s.D}, false, dev);
  return NfSylParams{r1.p, r2.p, a1.p, a2.p, bb.p, vv.p, r1.rs, r2.rs, a1.rs, a2.rs, bb.rs, vv.rs};
}

std::vector<unsigned char> flip_bytes(at::IntArrayRef flips) {
  std::vector<unsigned char> f(flips.size());
  for (size_t i = 0; i < flips.size(); ++i) f[i] = flips[i] != 0;
  return f;
}

void sylvester_fwd(const at::Tensor& z, const at::Tensor& R1, const at::Tensor& R2,
                   const at::Tensor& d1, const at::Tensor& d2, const at::Tensor& b,
                   const at::Tensor& V, at::IntArrayRef flips, const at::Tensor& zK,
                   const at::Tensor& ldj, const at::Tensor& saved) {
  const Dims s = chk_dims(z, V, flips);
  chk_dense(z, "z", {s.N, s.D});
  chk_dense(zK, "zK", {s.N, s.D});
  chk_dense(ldj, "ldj", {s.N});
  const bool keep = saved.numel() > 0 || s.N == 0;
  if (keep) chk_dense(saved, "saved", {s.N, s.K, s.D});
  const NfSylParams p = params_of(s, z, R1, R2, d1, d2, b, V);
  const auto f = flip_bytes(flips);
  nf_launch_sylvester_fwd(z.data_ptr<float>(), p, f.data(), zK.data_ptr<float>(),
                          ldj.data_ptr<float>(), keep ? saved.data_ptr<float>() : nullptr,
                          (int)s.N, (int)s.D, (int)s.K, (int)s.H, cur_stream());
}

void sylvester_bwd(const at::Tensor& saved, const at::Tensor& R1, const at::Tensor& R2,
                   const at::Tensor& d1, const at::Tensor& d2, const at::Tensor& b,
                   const at::Tensor& V, at::IntArrayRef flips, const at::Tensor& gz,
                   const at::Tensor& gl, const at::Tensor& dz, const at::Tensor& dR1,
                   const at::Tensor& dR2, const at::Tensor& dd1, const at::Tensor& dd2,
                   const at::Tensor& db, const at::Tensor& dV) {
  const Dims s = chk_dims(gz, V, flips);
  chk_dense(saved, "saved", {s.N, s.K, s.D});
  chk_dense(gz, "gz", {s.N, s.D});
  chk_dense(gl, "gl", {s.N});
  chk_dense(dz, "dz", {s.N, s.D});
  const NfSylParams p = params_of(s, gz, R1, R2, d1, d2, b, V);
  const auto dev = gz.device();
  const RowView r1 = row_view(dR1, "dR1", s.N, s.K, {s.P}, true, dev);
  const RowView r2 = row_view(dR2, "dR2", s.N, s.K, {s.P}, true, dev);
  const RowView a1 = row_view(dd1, "dd1", s.N, s.K, {s.D}, true, dev);
  const RowView a2 = row_view(dd2, "dd2", s.N, s.K, {s.D}, true, dev);
  const RowView bb = row_view(db, "db", s.N, s.K, {s.D}, true, dev);
  const RowView vv = row_view(dV, "dV", s.N, s.K, {s.H, s.D}, true, dev);
  const NfSylGrads g{r1.p, r2.p, a1.p, a2.p, bb.p, vv.p, r1.rs, r2.rs, a1.rs, a2.rs, bb.rs, vv.rs};
  const auto f = flip_bytes(flips);
  nf_launch_sylvester_bwd(saved.data_ptr<float>(), p, f.data(), gz.data_ptr<float>(),
                          gl.data_ptr<float>(), dz.data_ptr<float>(), g, (int)s.N, (int)s.D,
                          (int)s.K, (int)s.H, cur_stream());
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(vinf, m) {
  m.def("sylvester_fwd(Tensor z, Tensor R1, Tensor R2, Tensor d1, Tensor d2, Tensor b, Tensor V, "
        "int[] flips, Tensor(a!) zK, Tensor(b!) ldj, Tensor(c!) saved) -> ()");
  m.def("sylvester_bwd(Tensor saved, Tensor R1, Tensor R2, Tensor d1, Tensor d2, Tensor b, "
        "Tensor V, int[] flips, Tensor gz, Tensor gl, Tensor(a!) dz, Tensor(b!) dR1, "
        "Tensor(c!) dR2, Tensor(d!) dd1, Tensor(e!) dd2, Tensor(f!) db, Tensor(g!) dV) -> ()");
}

TORCH_LIBRARY_IMPL(vinf, CUDA, m) {
  m.impl("sylvester_fwd", &sylvester_fwd);
  m.impl("sylvester_bwd", &sylvester_bwd);
}
