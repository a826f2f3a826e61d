// Degree sweep: the sequential direction of a MADE-conditioned autoregressive flow (MAF sampling
// u -> x, IAF inverse y -> z) as ONE masked pass instead of D full MADE passes.
//
// made_degrees() gives every hidden layer sorted, non-decreasing degrees, so for the coordinate of
// degree t (t = 1 .. D, i = perm[t - 1])
//   * its two outputs m, s read a PREFIX h_L[:c(t)] of the last hidden layer (degrees < t),
//   * the hidden units of degree t form a contiguous range per layer, and read the first t
//     coordinates in degree order (layer 1) or a prefix of the layer below (degrees <= t).
// Walking t upwards is a forward substitution in which every in-mask weight is used exactly once
// per row; entries outside the masks are never read, so the weights need not be pre-masked.
//
// Mapping: a block of 256 threads owns a tile of R rows and keeps their state in LDS in fp32: x in
// DEGREE order (xs[r][t - 1], staged from v and overwritten coordinate by coordinate) and every
// hidden layer (hs[l][r][k], pre-filled with bias (+ context projection), overwritten by the
// activation). Each weight is read from global memory once per block and used for all R rows.
//   outputs of step t: the four waves take the 64-wide chunks of [0, c) round-robin, each lane
//     accumulating m and s of all R rows; a wave butterfly, then thread r adds the four wave
//     partials in wave order and applies the transform of coordinate i;
//   hidden units of degree t: one wave per unit, lanes strided over the inputs, wave butterfly.
// A row's sums therefore depend only on (c, t, lane, wave), never on R, on the row's place in the
// tile or on the batch size: a row's result is bitwise the same in any batch. No atomics.
// All arithmetic is fp32 with explicit fmaf; tanhf / expf / log1pf are the accurate library forms
// (errors feed forward through up to D dependent steps).
// The arguments are those of made_sweep_common.h, the staging, the hidden-unit phase and the final
// store the body fragments of made_sweep_phases.h (both also used by dsf_sweep.hip).
#include "made_sweep_common.h"

namespace {

using namespace nf_sweep;

__host__ __device__ inline long sweep_lds_floats(int R, int D, int H, int L) {
  return (long)R * ((long)D + (long)L * H) + D + NW * 2 * R;
}

// one coordinate: value v, conditioner outputs m, s -> x; returns the log-det share
__device__ __forceinline__ float sweep_transform(int kind, float p, float v, float m, float s,
                                                 float& x) {
  if (kind == 0) {             // MAF sampling: x = v exp(a) + m, a = p tanh(s / p)
    const float a = p * tanhf(s / p);
    x = fmaf(v, expf(a), m);
    return a;
  }
  if (kind == 1) {             // gated IAF inverse: v = g x + (1 - g) m, g = sigmoid(s + p)
    const float z = s + p;
    const float e = expf(-fabsf(z));
    const float g = z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    x = (v - (1.f - g) * m) / g;
    return log1pf(e) - fminf(z, 0.f);   // -logsigmoid(z)
  }
  const float c = p * tanhf(s);   // affine IAF inverse: v = x exp(c) + m
  x = (v - m) * expf(-c);
  return -c;
}

template <int R>
__global__ __launch_bounds__(NT) void made_sweep_kernel(const SweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int D = a.D, H = a.H, L = a.L;
  float* xs = lds;                          // [R][D], degree order
  float* hs = xs + (long)R * D;             // [L][R][H]
  float* part = hs + (long)L * R * H;       // [NW][2][R] wave partials of (m, s)
  int* pl = reinterpret_cast<int*>(part + NW * 2 * R);   // [D] perm
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long row0 = (long)blockIdx.x * R;
  const int W2 = D + 2;

#define NF_SWEEP_PHASE 1   // stage the tile
#include "made_sweep_phases.h"

  const float* hL = hs + (long)(L - 1) * R * H;
  float ldj = 0.f;
  for (int t = 1; t <= D; ++t) {
    const int i = pl[t - 1];
    const float bm = a.bo[i], bs = a.bo[i + D];
    // ---- outputs m, s of coordinate i over h_L[:c]
    {
      const int c = clampi(a.ubeg[(L - 1) * W2 + t], 0, H);
      const float* wm = a.Wo + (long)i * a.ldo;
      const float* ws = a.Wo + (long)(i + D) * a.ldo;
      float am[R], as[R];
#pragma unroll
      for (int r = 0; r < R; ++r) am[r] = as[r] = 0.f;
#pragma unroll 2
      for (int k = wid * 64 + lane; k < c; k += NT) {
        const float wmk = wm[k], wsk = ws[k];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float hv = hL[r * H + k];
          am[r] = fmaf(wmk, hv, am[r]);
          as[r] = fmaf(wsk, hv, as[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float sm = nf::wave_sum(am[r]), ss = nf::wave_sum(as[r]);
        if (lane == r) {
          part[(wid * 2 + 0) * R + r] = sm;
          part[(wid * 2 + 1) * R + r] = ss;
        }
      }
    }
    __syncthreads();
    if (tid < R) {
      float m = part[tid], s = part[R + tid];
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        m += part[(w * 2 + 0) * R + tid];
        s += part[(w * 2 + 1) * R + tid];
      }
      float xi;
      ldj += sweep_transform(a.kind, a.p, xs[tid * D + t - 1], bm + m, bs + s, xi);
      xs[tid * D + t - 1] = xi;
    }
    __syncthreads();
    // ---- hidden units of degree t, layer by layer
#define NF_SWEEP_PHASE 2
#include "made_sweep_phases.h"
  }

  if (tid < R && row0 + tid < a.B) a.ldj[row0 + tid] = ldj;
#define NF_SWEEP_PHASE 3   // store x
#include "made_sweep_phases.h"
}

template <int R>
void launch(const SweepArgs& a, hipStream_t stream) {
  const size_t bytes = sizeof(float) * sweep_lds_floats(R, a.D, a.H, a.L);
  static bool attr_set = false;
  if (!attr_set) {
    NF_HIP_CHECK(hipFuncSetAttribute((const void*)made_sweep_kernel<R>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));
    attr_set = true;
  }
  const long blocks = ((long)a.B + R - 1) / R;
  hipLaunchKernelGGL(made_sweep_kernel<R>, dim3((unsigned)blocks), dim3(NT), bytes, stream, a);
  NF_HIP_CHECK(hipGetLastError());
}

}  // namespace

int nf_made_sweep_rows(int D, int H, int L) {
  if (D < 1 || H < 1 || L < 1 || L > NF_MADE_SWEEP_MAX_HIDDEN) return 0;
  for (int R = kMaxRows; R >= 1; R >>= 1)
    if (sizeof(float) * sweep_lds_floats(R, D, H, L) <= (size_t)kLdsBudget) return R;
  return 0;
}

void nf_launch_made_sweep(const NfMadeSweep& s, hipStream_t stream) {
  SweepArgs a{};
  for (int l = 0; l < s.L; ++l) { a.W[l] = s.W[l]; a.b[l] = s.b[l]; a.ldw[l] = s.ldw[l]; }
  a.Wo = s.Wo; a.ldo = s.ldo; a.bo = s.bo;
  a.v = s.v; a.ldv = s.ldv; a.ctx = s.ctx; a.ldc = s.ldc;
  a.perm = s.perm; a.ubeg = s.ubeg;
  a.x = s.x; a.ldx = s.ldx; a.ldj = s.ldj;
  a.B = s.B; a.D = s.D; a.H = s.H; a.L = s.L; a.kind = s.kind; a.p = s.param;
  switch (nf_made_sweep_rows(s.D, s.H, s.L)) {
    case 8: launch<8>(a, stream); break;
    case 4: launch<4>(a, stream); break;
    case 2: launch<2>(a, stream); break;
    case 1: launch<1>(a, stream); break;
    default:
      nf_throw_hip_error(hipErrorInvalidValue, "made_sweep: shape exceeds the LDS budget",
                         __FILE__, __LINE__);
  }
}
