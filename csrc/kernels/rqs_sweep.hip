// RQS degree sweep: the sequential direction of a MADE-conditioned rational-quadratic spline layer
// (RQSAutoregressive, y -> z: solve T(z) = y coordinate by coordinate) as ONE masked pass instead
// of D full MADE passes, each followed by the spline inverse of one coordinate.
//
// The walk t = 1 .. D, the row tile in LDS, the staging, the hidden-unit phase and the store are
// those of made_sweep.hip (made_sweep_common.h, made_sweep_phases.h); the kernel is dsf_sweep.hip
// with another output count and a closed-form transform:
//   * the coordinate i = perm[t - 1] has 3K - 1 conditioner outputs
//       p_k = bo[k D + i] + Wo[k D + i, :c(t)] . h_L[:c(t)],  k = 0 .. 3K - 2,
//     plane-major as MADE(out_mult = 3K - 1) emits them (planes [0, K) unnormalised widths,
//     [K, 2K) heights, [2K, 3K - 1) interior derivatives). The four waves take the BINS
//     round-robin; a wave holds the width, height and derivative rows of its bin at once (the
//     derivative row exists for k < K - 1 only, a wave-uniform predicate), so one h_L value read
//     from LDS serves 3 R fmas. Every dot product is a lane-strided sum over [0, c) and a wave
//     butterfly: its order depends on (c, lane) only. The results are staged in LDS as
//     st[r][3K - 1], bias included, in plane order: the element code of rqs_elem.h reads st as it
//     reads a params row with one element;
//   * the transform is the inverse spline of rqs_elem.h (a quadratic: no root search). Every row
//     has a fixed group of kGroup = 32 lanes (half a wave), and lane k of the group owns bin k:
//     one exp per softmax per lane, max and sum by xor shuffles and the knots by an exclusive
//     scan inside the 32-lane half, the bin by a ballot of `lower y-knot <= v` and a popcount,
//     the bin's values by shuffles from that lane, then rqs_eval<true> in every lane:
//     z = xk + theta w and ldj -= log(s^2 P / den^2). Every trip count is compile-time
//     (log2 KMAX shuffle steps) and no shuffle leaves a row's half-wave. Nothing diverges: a v
//     outside (-bound, bound), or a NaN, evaluates the spline too (every comparison with a NaN is
//     false, which leaves bin 0) and the result is replaced by the identity with ldj share 0.
//     -DRQS_SWEEP_REDUNDANT builds the form in which every lane of the group computes the whole
//     element from st instead (rqs_find_bin<KMAX, true>: nothing is exchanged); it takes 5 %
//     longer at (B, D, H, K) = (4096, 256, 512, 8), 7 % at (8192, 1024, 1024, 8) and 17 % at
//     K = 32 (docs/PERF_NOTES.md, "RQS degree sweep").
// A row's (z, ldj) depends on its own data, (D, H, L, K, bound) and the plan only: bitwise the
// same in any batch, at any place in its tile and across launches. No atomics.
//
// exp / log / rcp / sqrt are the accurate library forms (EW_ACCURATE_MATH of elementwise_flow.h),
// unlike dsf_sweep.hip: over the cases of tests/test_rqs_sweep_gpu.py the fast device intrinsics
// are further from the fp64 result in this form (worst ratio 3.3 against 2.3) and a launch is
// only 3 % faster with them (docs/PERF_NOTES.md, "RQS degree sweep"). -DRQS_SWEEP_FAST_MATH builds
// the fast intrinsics for that comparison.
#ifndef RQS_SWEEP_FAST_MATH
#define EW_ACCURATE_MATH 1
#endif
#include "rqs_elem.h"
#include "made_sweep_common.h"

namespace {

using namespace nf_sweep;
using namespace nf;

constexpr int kGroup = 32;                 // lanes per row in the transform; K <= kGroup
static_assert(kMaxRows * kGroup <= NT, "every row of a tile needs its own lane group");

struct RqsSweepArgs {
  SweepArgs s;   // kind and p are unused
  int K;
  float bound;
};

__host__ __device__ inline long rqs_sweep_lds_floats(int R, int D, int H, int L, int K) {
  return (long)R * ((long)D + (long)L * H + 3L * K - 1) + D;
}

#ifndef RQS_SWEEP_REDUNDANT
// Sum / maximum over the lanes [0, KMAX) of a 32-lane group; lanes >= KMAX hold the neutral value
// and end with a partial result nobody reads. xor masks < 32 never leave the half-wave.
template <int KMAX>
__device__ __forceinline__ float grp_max(float v) {
#pragma unroll
  for (int m = KMAX / 2; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}
template <int KMAX>
__device__ __forceinline__ float grp_sum(float v) {
#pragma unroll
  for (int m = KMAX / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
// Exclusive prefix sum over the lanes of a 32-lane group (lanes >= K contribute 0).
template <int KMAX>
__device__ __forceinline__ float grp_excl_scan(float v, int gl) {
  float x = __shfl_up(v, 1, kGroup);
  x = gl >= 1 ? x : 0.f;
#pragma unroll
  for (int d = 1; d < KMAX; d <<= 1) {
    const float t = __shfl_up(x, d, kGroup);
    x += gl >= d ? t : 0.f;
  }
  return x;
}

// The bin of v among the y-knots with lane gl of the group owning bin gl; every lane returns the
// same RqsBin (sw / sh / cw / ch are the backward's and stay 0).
template <int KMAX>
__device__ __forceinline__ void rqs_find_bin_coop(const float* __restrict__ p, int K, float bound,
                                                  float v, int gl, int lane, RqsBin& bn) {
  const bool act = gl < K;
  const float uw = act ? p[gl] : -INFINITY, uh = act ? p[K + gl] : -INFINITY;
  const float mw = grp_max<KMAX>(uw), mh = grp_max<KMAX>(uh);
  const float ew = act ? EW_EXP(uw - mw) : 0.f, eh = act ? EW_EXP(uh - mh) : 0.f;
  const float iw = EW_RCP(grp_sum<KMAX>(ew)), ih = EW_RCP(grp_sum<KMAX>(eh));
  const float c2 = 2.0f * bound, cm = 1.0f - (float)K * RQS_MIN;
  const float wk = act ? c2 * fmaf(cm, ew * iw, RQS_MIN) : 0.f;
  const float hk = act ? c2 * fmaf(cm, eh * ih, RQS_MIN) : 0.f;
  const float kx = grp_excl_scan<KMAX>(wk, gl) - bound;   // lower knots of bin gl
  const float ky = grp_excl_scan<KMAX>(hk, gl) - bound;
  // the knots increase, so the bins whose lower knot is <= v are a prefix; a NaN leaves bin 0
  const unsigned long long m = __ballot(act && (gl == 0 || v >= ky));
  const int kb = __popc((unsigned)(m >> (lane & 32))) - 1;
  bn.k = kb;
  bn.xk = __shfl(kx, kb, kGroup);
  bn.w = __shfl(wk, kb, kGroup);
  bn.yk = __shfl(ky, kb, kGroup);
  bn.h = __shfl(hk, kb, kGroup);
  bn.sw = bn.sh = bn.cw = bn.ch = 0.f;
  const bool first = kb == 0, last = kb == K - 1;
  const float ud0 = p[2 * K + (first ? 0 : kb - 1)];
  const float ud1 = p[2 * K + (last ? K - 2 : kb)];
  bn.u0 = ud0 + RQS_C0;
  bn.u1 = ud1 + RQS_C0;
  bn.d0 = first ? 1.0f : rqs_deriv(ud0);
  bn.d1 = last ? 1.0f : rqs_deriv(ud1);
}
#endif

template <int R, int KMAX>
__global__ __launch_bounds__(NT) void rqs_sweep_kernel(const RqsSweepArgs ra) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const SweepArgs& a = ra.s;
  const int D = a.D, H = a.H, L = a.L, K = ra.K;
  const float bound = ra.bound;
  const int P = 3 * K - 1;
  float* xs = lds;                          // [R][D], degree order
  float* hs = xs + (long)R * D;             // [L][R][H]
  float* st = hs + (long)L * R * H;         // [R][3K - 1] conditioner outputs of the step
  int* pl = reinterpret_cast<int*>(st + (long)R * P);   // [D] perm
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long row0 = (long)blockIdx.x * R;
  const int W2 = D + 2;
  // the row this lane transforms; with R < 8 the spare groups repeat rows and store nothing
  const int grp = tid / kGroup, gl = tid % kGroup;
  const int rr = grp % R;
  const bool owner = grp < R && gl == 0;

#define NF_SWEEP_PHASE 1   // stage the tile
#include "made_sweep_phases.h"

  const float* hL = hs + (long)(L - 1) * R * H;
  float ldj = 0.f;
  for (int t = 1; t <= D; ++t) {
    const int i = pl[t - 1];
    const float v = xs[rr * D + t - 1];   // read before the step's first barrier, replaced after it
    // ---- the 3K - 1 outputs of coordinate i over h_L[:c]: a wave per bin, three rows at once
    {
      const int c = clampi(a.ubeg[(L - 1) * W2 + t], 0, H);
      for (int k = wid; k < K; k += NW) {
        const bool hasd = k < K - 1;   // wave-uniform: the last bin has no interior derivative
        const long rw = (long)k * D + i, rh = rw + (long)K * D, rd = rh + (long)K * D;
        const float* ww = a.Wo + rw * a.ldo;
        const float* wh = a.Wo + rh * a.ldo;
        const float* wd = a.Wo + (hasd ? rd : rw) * a.ldo;   // a row that exists; unused if !hasd
        float aw[R], ah[R], ad[R];
#pragma unroll
        for (int r = 0; r < R; ++r) aw[r] = ah[r] = ad[r] = 0.f;
#pragma unroll 2
        for (int j = lane; j < c; j += 64) {
          const float wwj = ww[j], whj = wh[j], wdj = wd[j];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const float hv = hL[r * H + j];
            aw[r] = fmaf(wwj, hv, aw[r]);
            ah[r] = fmaf(whj, hv, ah[r]);
            ad[r] = fmaf(wdj, hv, ad[r]);
          }
        }
        const float bw = a.bo[rw], bh = a.bo[rh], bd = a.bo[hasd ? rd : rw];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float sw = nf::wave_sum(aw[r]), sh = nf::wave_sum(ah[r]),
                      sd = nf::wave_sum(ad[r]);
          if (lane == r) {
            st[r * P + k] = bw + sw;
            st[r * P + K + k] = bh + sh;
            if (hasd) st[r * P + 2 * K + k] = bd + sd;
          }
        }
      }
    }
    __syncthreads();
    // ---- inverse spline of row rr by its lane group
    {
      RqsBin bn;
#ifdef RQS_SWEEP_REDUNDANT
      float smw[KMAX], smh[KMAX];
      rqs_find_bin<KMAX, true>(st + rr * P, 0u, 1u, K, bound, v, smw, smh, bn);
#else
      rqs_find_bin_coop<KMAX>(st + rr * P, K, bound, v, gl, lane, bn);
#endif
      RqsEval ev;
      rqs_eval<true>(bn, v, ev);
      const bool inside = v > -bound && v < bound;   // linear tails (and NaN): identity, ldj 0
      const float z = inside ? fmaf(ev.th, bn.w, bn.xk) : v;
      const float lg = EW_LOG(ev.s * ev.s * ev.P * ev.rden * ev.rden);   // log dy/dx at z
      ldj -= inside ? lg : 0.f;
      if (owner) xs[rr * D + t - 1] = z;
    }
    __syncthreads();
    // ---- hidden units of degree t, layer by layer
#define NF_SWEEP_PHASE 2
#include "made_sweep_phases.h"
  }

  if (owner && row0 + rr < a.B) a.ldj[row0 + rr] = ldj;
#define NF_SWEEP_PHASE 3   // store x
#include "made_sweep_phases.h"
}

template <int R, int KMAX>
void launch(const RqsSweepArgs& a, hipStream_t stream) {
  const size_t bytes = sizeof(float) * rqs_sweep_lds_floats(R, a.s.D, a.s.H, a.s.L, a.K);
  static bool attr_set = false;
  if (!attr_set) {
    NF_HIP_CHECK(hipFuncSetAttribute((const void*)rqs_sweep_kernel<R, KMAX>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));
    attr_set = true;
  }
  const long blocks = ((long)a.s.B + R - 1) / R;
  hipLaunchKernelGGL((rqs_sweep_kernel<R, KMAX>), dim3((unsigned)blocks), dim3(NT), bytes, stream,
                     a);
  NF_HIP_CHECK(hipGetLastError());
}

template <int KMAX>
void launch_rows(int R, const RqsSweepArgs& a, hipStream_t stream) {
  switch (R) {
    case 8: launch<8, KMAX>(a, stream); break;
    case 4: launch<4, KMAX>(a, stream); break;
    case 2: launch<2, KMAX>(a, stream); break;
    case 1: launch<1, KMAX>(a, stream); break;
    default:
      nf_throw_hip_error(hipErrorInvalidValue, "rqs_sweep: shape exceeds the LDS budget",
                         __FILE__, __LINE__);
  }
}

}  // namespace

int nf_rqs_sweep_rows(int D, int H, int L, int K) {
  if (D < 1 || H < 1 || L < 1 || L > NF_MADE_SWEEP_MAX_HIDDEN || K < 2 || K > 32) return 0;
  for (int R = kMaxRows; R >= 1; R >>= 1)
    if (sizeof(float) * rqs_sweep_lds_floats(R, D, H, L, K) <= (size_t)kLdsBudget) return R;
  return 0;
}

void nf_launch_rqs_sweep(const NfMadeSweep& s, int K, float bound, hipStream_t stream) {
  RqsSweepArgs d{};
  SweepArgs& a = d.s;
  for (int l = 0; l < s.L; ++l) { a.W[l] = s.W[l]; a.b[l] = s.b[l]; a.ldw[l] = s.ldw[l]; }
  a.Wo = s.Wo; a.ldo = s.ldo; a.bo = s.bo;
  a.v = s.v; a.ldv = s.ldv; a.ctx = s.ctx; a.ldc = s.ldc;
  a.perm = s.perm; a.ubeg = s.ubeg;
  a.x = s.x; a.ldx = s.ldx; a.ldj = s.ldj;
  a.B = s.B; a.D = s.D; a.H = s.H; a.L = s.L;
  d.K = K;
  d.bound = bound;
  const int R = nf_rqs_sweep_rows(s.D, s.H, s.L, K);
  if (K <= 8) launch_rows<8>(R, d, stream);
  else if (K <= 16) launch_rows<16>(R, d, stream);
  else launch_rows<32>(R, d, stream);
}
