// DSF degree sweep: the inverse of a MADE-conditioned deep sigmoidal flow layer
// (DSFAutoregressive.inverse, y -> z) as ONE masked pass instead of D full MADE passes, each
// followed by a root solve of one coordinate.
//
// The walk t = 1 .. D, the row tile in LDS, the staging, the hidden-unit phase and the store are
// those of made_sweep.hip (made_sweep_common.h, made_sweep_phases.h). Two things differ:
//   * the coordinate i = perm[t - 1] has 3U conditioner outputs
//       p_k = bo[k D + i] + Wo[k D + i, :c(t)] . h_L[:c(t)],  k = 0 .. 3U - 1,
//     plane-major as MADE(out_mult = 3U) emits them (planes [0, U) raw slopes, [U, 2U) shifts,
//     [2U, 3U) mixture logits). The four waves take the UNITS round-robin; a wave holds the three
//     output rows of its unit at once, so one h_L value read from LDS serves 3 R fmas. Every dot
//     product is a lane-strided sum over [0, c) and a wave butterfly: its order depends on
//     (c, lane) only. The 3U x R results are staged in LDS as st[r][3U], bias included;
//   * the transform is the root solve of dsf_elem.h. Every row has a fixed group of kGroup = 32
//     lanes (half a wave). Each lane of the group builds the row's units from st and evaluates one
//     interior point of the bracket; y(x) is monotone, so a ballot and a popcount give the
//     sub-interval and every round shrinks the bracket 33x: kRounds = 8 rounds replace the 40
//     halvings of the one-lane solve (33^8 > 2^40). Every lane of a group computes the same
//     (lo, hi) from the same ballot, so no value is exchanged. Every loop has a compile-time trip
//     count; a comparison with a NaN is false, so a NaN only moves an end of its own row's bracket.
//     ldj is evaluated at the recovered z with the full three-logsumexp form (dsf_eval).
//     -DDSF_SWEEP_ONE_LANE builds the one-lane fixed-trip bisection (dsf_solve) instead, for the
//     comparison in docs/PERF_NOTES.md ("DSF degree sweep").
// A row's (z, ldj) depends on its own data, (D, H, L, U) and the plan only: bitwise the same in any
// batch, at any place in its tile and across launches. No atomics.
//
// exp / log are the fast device intrinsics of the element-wise kernels (EW_EXP / EW_LOG): over the
// cases of tests/test_dsf_sweep_gpu.py they stay as close to the fp64 result as the accurate
// library forms (worst ratio 2.2 against 2.7) and a launch is 1.3x faster (docs/PERF_NOTES.md,
// "DSF degree sweep"). -DDSF_SWEEP_ACCURATE_MATH builds the accurate forms for that comparison.
#ifdef DSF_SWEEP_ACCURATE_MATH
#define EW_ACCURATE_MATH 1
#endif
#include "dsf_elem.h"
#include "made_sweep_common.h"

namespace {

using namespace nf_sweep;
using namespace nf;

constexpr int kGroup = 32;                 // lanes per row in the root solve
constexpr int kRounds = 8;                 // (kGroup + 1)^kRounds > 2^DSF_BISECT
static_assert(kMaxRows * kGroup <= NT, "every row of a tile needs its own lane group");

struct DsfSweepArgs {
  SweepArgs s;   // kind and p are unused
  int U;
};

__host__ __device__ inline long dsf_sweep_lds_floats(int R, int D, int H, int L, int U) {
  return (long)R * ((long)D + (long)L * H + 3L * U) + D;
}

// Interior point k of kGroup + 1 equal parts of [lo, lo + w]; non-decreasing in k.
__device__ __forceinline__ float part_point(float lo, float w, int k) {
  return fmaf(w, (float)k * (1.0f / (kGroup + 1)), lo);
}

template <int R, int UMAX>
__global__ __launch_bounds__(NT) void dsf_sweep_kernel(const DsfSweepArgs da) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const SweepArgs& a = da.s;
  const int D = a.D, H = a.H, L = a.L, U = da.U;
  const int P = 3 * U;
  float* xs = lds;                          // [R][D], degree order
  float* hs = xs + (long)R * D;             // [L][R][H]
  float* st = hs + (long)L * R * H;         // [R][3U] conditioner outputs of the step
  int* pl = reinterpret_cast<int*>(st + (long)R * P);   // [D] perm
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long row0 = (long)blockIdx.x * R;
  const int W2 = D + 2;
  // the row this lane helps to solve; with R < 8 the spare groups repeat rows and store nothing
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
    // ---- the 3U outputs of coordinate i over h_L[:c]: a wave per unit, three rows at once
    {
      const int c = clampi(a.ubeg[(L - 1) * W2 + t], 0, H);
      for (int h = wid; h < U; h += NW) {
        const long ra = (long)h * D + i, rb = ra + (long)U * D, rw = rb + (long)U * D;
        const float* wa = a.Wo + ra * a.ldo;
        const float* wb = a.Wo + rb * a.ldo;
        const float* ww = a.Wo + rw * a.ldo;
        float aa[R], ab[R], aw[R];
#pragma unroll
        for (int r = 0; r < R; ++r) aa[r] = ab[r] = aw[r] = 0.f;
#pragma unroll 2
        for (int k = lane; k < c; k += 64) {
          const float wak = wa[k], wbk = wb[k], wwk = ww[k];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const float hv = hL[r * H + k];
            aa[r] = fmaf(wak, hv, aa[r]);
            ab[r] = fmaf(wbk, hv, ab[r]);
            aw[r] = fmaf(wwk, hv, aw[r]);
          }
        }
        const float ba = a.bo[ra], bb = a.bo[rb], bw = a.bo[rw];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float sa = nf::wave_sum(aa[r]), sb = nf::wave_sum(ab[r]),
                      sw = nf::wave_sum(aw[r]);
          if (lane == r) {
            st[r * P + h] = ba + sa;
            st[r * P + U + h] = bb + sb;
            st[r * P + 2 * U + h] = bw + sw;
          }
        }
      }
    }
    __syncthreads();
    // ---- root solve of row rr by its lane group, then ldj at the root
    {
      DsfUnits<UMAX> u;
      dsf_load<UMAX>(st + rr * P, 0u, 1u, U, u);
#ifdef DSF_SWEEP_ONE_LANE
      const float z = dsf_solve<UMAX>(u, U, v);
#else
      float lo, hi;
      dsf_bracket<UMAX>(u, U, v, lo, hi);
#pragma unroll 1
      for (int it = 0; it < kRounds; ++it) {
        const float w = hi - lo;
        const bool below = dsf_value<UMAX>(u, U, part_point(lo, w, gl + 1)) < v;
        const unsigned long long m = __ballot(below);
        const int n = __popc((unsigned)(m >> (lane & 32)));   // points of this row below the root
        const float nlo = n == 0 ? lo : part_point(lo, w, n);
        const float nhi = n == kGroup ? hi : part_point(lo, w, n + 1);
        lo = nlo;
        hi = nhi;
      }
      const float z = 0.5f * lo + 0.5f * hi;
#endif
      DsfEval<UMAX> ev;
      dsf_eval<UMAX>(u, U, z, ev);
      ldj -= ev.L;
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

template <int R, int UMAX>
void launch(const DsfSweepArgs& a, hipStream_t stream) {
  const size_t bytes = sizeof(float) * dsf_sweep_lds_floats(R, a.s.D, a.s.H, a.s.L, a.U);
  static bool attr_set = false;
  if (!attr_set) {
    NF_HIP_CHECK(hipFuncSetAttribute((const void*)dsf_sweep_kernel<R, UMAX>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));
    attr_set = true;
  }
  const long blocks = ((long)a.s.B + R - 1) / R;
  hipLaunchKernelGGL((dsf_sweep_kernel<R, UMAX>), dim3((unsigned)blocks), dim3(NT), bytes, stream,
                     a);
  NF_HIP_CHECK(hipGetLastError());
}

template <int UMAX>
void launch_rows(int R, const DsfSweepArgs& a, hipStream_t stream) {
  switch (R) {
    case 8: launch<8, UMAX>(a, stream); break;
    case 4: launch<4, UMAX>(a, stream); break;
    case 2: launch<2, UMAX>(a, stream); break;
    case 1: launch<1, UMAX>(a, stream); break;
    default:
      nf_throw_hip_error(hipErrorInvalidValue, "dsf_sweep: shape exceeds the LDS budget",
                         __FILE__, __LINE__);
  }
}

}  // namespace

int nf_dsf_sweep_rows(int D, int H, int L, int U) {
  if (D < 1 || H < 1 || L < 1 || L > NF_MADE_SWEEP_MAX_HIDDEN || U < 1 || U > 32) return 0;
  for (int R = kMaxRows; R >= 1; R >>= 1)
    if (sizeof(float) * dsf_sweep_lds_floats(R, D, H, L, U) <= (size_t)kLdsBudget) return R;
  return 0;
}

void nf_launch_dsf_sweep(const NfMadeSweep& s, int U, hipStream_t stream) {
  DsfSweepArgs d{};
  SweepArgs& a = d.s;
  for (int l = 0; l < s.L; ++l) { a.W[l] = s.W[l]; a.b[l] = s.b[l]; a.ldw[l] = s.ldw[l]; }
  a.Wo = s.Wo; a.ldo = s.ldo; a.bo = s.bo;
  a.v = s.v; a.ldv = s.ldv; a.ctx = s.ctx; a.ldc = s.ldc;
  a.perm = s.perm; a.ubeg = s.ubeg;
  a.x = s.x; a.ldx = s.ldx; a.ldj = s.ldj;
  a.B = s.B; a.D = s.D; a.H = s.H; a.L = s.L;
  d.U = U;
  const int R = nf_dsf_sweep_rows(s.D, s.H, s.L, U);
  if (U <= 8) launch_rows<8>(R, d, stream);
  else if (U <= 16) launch_rows<16>(R, d, stream);
  else launch_rows<32>(R, d, stream);
}
