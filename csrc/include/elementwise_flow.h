// Shared frame of the element-wise flow transforms (spline.hip, dsf.hip): an element-wise,
// conditioner-parameterised monotone map over x [B, D] with PLANE-major params [B, planes * D]
// in fp32 or bf16 (column p*D + j is plane p of element j, so adjacent lanes read adjacent
// columns of one plane and every plane load is coalesced).
//
// One wave64 owns one row; 4 rows per 256-thread block; lanes stride over j; ldj is a 64-wide
// shuffle sum, so there are no atomics and every result is bitwise repeatable. The backward
// saves nothing and writes every dparams column.
//
// A transform plugs in with an Op: a trivially copyable policy type templated on
// <NMAX, INVERSE> (NMAX in {8, 16, 32} bounds the per-element count n, whose loops are fully
// unrolled) that carries the transform's scalar arguments, the count first, and has
//   static constexpr const char* NEED          what valid() asks for, for the error text
//   bool valid() const                         the scalars are in range
//   int planes() const                         planes per element
//   float fwd_elem(pr, j, D, v, acc) const     one element; adds its log dy/dx to acc
//   float bwd_elem(pr, dpr, j, D, v, g, gl) const   writes the element's planes() parameter
//                                              gradients, returns the input's gradient
// and two launchers that call ew_launch<Op>(...) with EwFwd / EwBwd. fwd_elem / bwd_elem hold
// the element code itself (one inlining layer below the kernel, as before the frame was
// shared): so built, the 48 kernels of spline.hip and dsf.hip compile to the
// instruction streams they had as separate kernels (profiles/r12/elementwise_isa.txt).
#pragma once

#include "nf_common.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

// The element math is __host__ __device__ so it can also be exercised by a host program; the
// fast intrinsics exist on the device only. A unit that defines EW_ACCURATE_MATH before its first
// include gets the accurate library forms on the device too (dsf_sweep.hip, for its accuracy
// comparison).
#if defined(__HIP_DEVICE_COMPILE__) && !defined(EW_ACCURATE_MATH)
#define EW_EXP(v) __expf(v)
#define EW_LOG(v) __logf(v)
#define EW_RCP(v) __builtin_amdgcn_rcpf(v)
#define EW_SQRT(v) __builtin_amdgcn_sqrtf(v)
#else
#define EW_EXP(v) expf(v)
#define EW_LOG(v) logf(v)
#define EW_RCP(v) (1.0f / (v))
#define EW_SQRT(v) sqrtf(v)
#endif
#define EW_HD __host__ __device__ __forceinline__

namespace nf {

// Accesses inside a params row are (wave-uniform row pointer)[32-bit column]; the column walks
// plane by plane (+= D), so no per-plane address is kept live across the loop over j.
EW_HD float ew_ld(const float* p, unsigned j) { return p[j]; }
EW_HD float ew_ld(const bf16_t* p, unsigned j) {
  union { uint32_t u; float f; } c;
  c.u = ((uint32_t)p[j]) << 16;
  return c.f;
}
EW_HD void ew_st(float* p, unsigned j, float v) { p[j] = v; }
EW_HD void ew_st(bf16_t* p, unsigned j, float v) {
  const __hip_bfloat16 h = __float2bfloat16(v);
  p[j] = *reinterpret_cast<const bf16_t*>(&h);
}

// x [B, D] is the input of the direction taken (the inverse reads y here), y [B, D] the output,
// ldj [B] the row sum of log dy/dx (inverse: minus that), initialised or accumulated into.
template <typename Op, typename TP>
__global__ void __launch_bounds__(256) ew_fwd_kernel(
    const TP* __restrict__ params, const float* __restrict__ x, float* __restrict__ y,
    float* __restrict__ ldj, int B, int D, Op op, int ldj_init) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const TP* p_r = params + row * (long)op.planes() * D;
  const float* x_r = x + row * D;
  float* y_r = y + row * D;
  float acc = 0.f;
#pragma unroll 1
  for (int j = lane; j < D; j += 64) y_r[j] = op.fwd_elem(p_r, j, (unsigned)D, x_r[j], acc);
  acc = wave_sum(acc);
  if (lane == 0) ldj[row] = ldj_init ? acc : ldj[row] + acc;
}

// g_out [B, D], g_ldj [B]: upstream gradients of the direction's output and ldj.
// dparams [B, planes D] in the dtype of params (every column written), gx [B, D].
template <typename Op, typename TP>
__global__ void __launch_bounds__(256) ew_bwd_kernel(
    const TP* __restrict__ params, const float* __restrict__ x, const float* __restrict__ g_out,
    const float* __restrict__ g_ldj, TP* __restrict__ dparams, float* __restrict__ gx, int B,
    int D, Op op) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const long prow = row * (long)op.planes() * D;
  const float gl = g_ldj[row];
#pragma unroll 1
  for (int j = lane; j < D; j += 64)
    gx[row * D + j] = op.bwd_elem(params + prow, dparams + prow, j, (unsigned)D, x[row * D + j],
                                  g_out[row * D + j], gl);
}

// The tensors of one pass besides params; launch<TP> starts its kernel for an Op.
struct EwFwd {
  const float* x;
  float *y, *ldj;
  int ldj_init;
  template <typename TP, typename Op>
  void launch(Op op, const void* params, int B, int D, dim3 grid, hipStream_t stream) const {
    hipLaunchKernelGGL((ew_fwd_kernel<Op, TP>), grid, dim3(256), 0, stream, (const TP*)params, x,
                       y, ldj, B, D, op, ldj_init);
  }
};

struct EwBwd {
  const float *x, *g_out, *g_ldj;
  void* dparams;
  float* gx;
  template <typename TP, typename Op>
  void launch(Op op, const void* params, int B, int D, dim3 grid, hipStream_t stream) const {
    hipLaunchKernelGGL((ew_bwd_kernel<Op, TP>), grid, dim3(256), 0, stream, (const TP*)params, x,
                       g_out, g_ldj, (TP*)dparams, gx, B, D, op);
  }
};

// Host dispatch of one pass over NMAX in {8, 16, 32} x direction x params dtype. n is the Op's
// first scalar, rest... the others.
template <typename Pass, typename Op>
void ew_launch_op(const Pass& pass, Op op, const void* params, int params_is_bf16, int B, int D,
                  hipStream_t stream) {
  const dim3 grid((B + 3) / 4);
  if (params_is_bf16) pass.template launch<bf16_t>(op, params, B, D, grid, stream);
  else pass.template launch<float>(op, params, B, D, grid, stream);
}

template <template <int, bool> class OpT, int NMAX, typename Pass, typename... Sc>
void ew_launch_nmax(const Pass& pass, const void* params, int params_is_bf16, int B, int D,
                    int inverse, hipStream_t stream, Sc... sc) {
  if (inverse) ew_launch_op(pass, OpT<NMAX, true>{sc...}, params, params_is_bf16, B, D, stream);
  else ew_launch_op(pass, OpT<NMAX, false>{sc...}, params, params_is_bf16, B, D, stream);
}

template <template <int, bool> class OpT, typename Pass, typename... Sc>
void ew_launch(const char* what, const Pass& pass, const void* params, int params_is_bf16, int B,
               int D, int inverse, hipStream_t stream, int n, Sc... rest) {
  if (B <= 0 || D <= 0) return;
  const OpT<32, false> probe{n, rest...};
  // columns inside a params row are 32-bit offsets (byte offsets stay below 2^31)
  if (!probe.valid() || (long)probe.planes() * D >= (1L << 29)) {
    fprintf(stderr, "%s: need %s and planes * D < 2^29\n", what, probe.NEED);
    abort();
  }
  const int bf = params_is_bf16;
  if (n <= 8) ew_launch_nmax<OpT, 8>(pass, params, bf, B, D, inverse, stream, n, rest...);
  else if (n <= 16) ew_launch_nmax<OpT, 16>(pass, params, bf, B, D, inverse, stream, n, rest...);
  else ew_launch_nmax<OpT, 32>(pass, params, bf, B, D, inverse, stream, n, rest...);
  NF_HIP_CHECK(hipGetLastError());
}

}  // namespace nf
