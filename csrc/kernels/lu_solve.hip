// Triangular solves against a packed LU (or Cholesky-type) factor, one launch per call:
//   mode LU,    transpose 0:  s[:, perm[i]] = y[:, i] - b[i];  L z = s;  U x = z;  store x
//   mode LU,    transpose 1:  U^T q = gx;  L^T g = q;  store g[:, perm]            (W^-T gx)
//   mode LOWER, transpose 0:  s as above;  T x = s;  store x      (T = lower triangle with diagonal)
//   mode LOWER, transpose 1:  T^T g = gx;  store g[:, perm]
// with W = (L U)[perm, :], L = strict lower triangle of A with an implied unit diagonal, U = upper
// triangle of A with its diagonal. The permutation and the bias are applied while staging and
// storing; z never leaves LDS.
//
// The kernel reads ONE orientation of the factor, M ("equation-major"): M[k][i] is the coefficient
// of unknown k in equation i, so the 64 lanes of a wave, one equation each, read M[k][j0 .. j0+63]
// as one coalesced 256-byte segment. The launcher passes At = A^T for transpose 0 and A itself for
// transpose 1. A solve that walks the unknowns upwards reads M[k][i] with k < i (k <= i with a
// diagonal), one that walks downwards k > i (k >= i); nothing else is ever loaded, so the unused
// triangle of a LOWER factor may hold anything and the unit diagonal of L is never read.
//
// Mapping: a block of 256 threads (4 waves) owns a tile of R rows and keeps their vectors in LDS
// in fp32, padded with zeros to a multiple of 64 coordinates. A solve walks the triangle in
// 64-wide panels; per panel
//   off-panel: lane = equation i of the panel; the unknowns already solved are dealt to the four
//     waves in groups of four (wave w takes k = 16 t + 4 w .. + 3 from the panel's far edge), each
//     lane accumulating its equation's dot product for all R rows with fmaf, the row values coming
//     as LDS broadcasts; the four wave partials go to LDS;                          -- barrier 1
//   in-panel: wave w takes the rows r = w, w + 4, ..: rhs = s - ((p0 + p1) + (p2 + p3)), then the
//     64 x 64 substitution out of an LDS copy of the diagonal tile: 64 steps of v_readlane, an IEEE
//     division by the diagonal (skipped for the unit factor) and one fmaf; x back to LDS -- barrier 2
// A row's sums depend only on (D, panel, lane, wave), never on R, on the row's place in the tile
// or on the batch size: a row's result is bitwise the same in any batch. Every trip count is fixed
// by D; a NaN or a zero diagonal gives inf / NaN and nothing else. No atomics, no scratch.
#include "nf_common.h"

#ifndef NF_LU_MAX_ROWS
#define NF_LU_MAX_ROWS 16
#endif

namespace {

constexpr int NT = 256;            // threads per block (4 waves)
constexpr int NW = NT / 64;
constexpr int PW = 64;             // panel width
constexpr int kLdsBudget = 81920;  // bytes per block, as the degree sweeps: two blocks per CU
constexpr int kMaxRows = NF_LU_MAX_ROWS;
constexpr int kMaxD = 2048;

struct LuArgs {
  const float* M; long ldm;   // equation-major factor (see above)
  const float* y; long ldy;
  const int* perm;            // [D] or null
  const float* bias;          // [D] or null (transpose 0 only)
  float* x; long ldx;
  int B, D, mode, transpose;
};

__host__ __device__ inline int padded(int D) { return (D + PW - 1) / PW * PW; }

__host__ __device__ inline long lds_floats(int R, int D) {
  return (long)R * padded(D) + (long)NW * R * PW + PW * PW;
}

__device__ __forceinline__ float lane_value(float v, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

// One triangular solve in place in xs [R][Dp]. UP: unknowns 0 .. D-1 (M's upper triangle),
// otherwise D-1 .. 0 (its lower triangle); UNIT: the diagonal is 1 and not read.
template <int R, bool UP, bool UNIT>
__device__ __forceinline__ void tri_solve(const LuArgs& a, float* xs, float* part, float* tile,
                                          int Dp) {
  constexpr int RW = (R + NW - 1) / NW;   // rows a wave substitutes
  const int D = a.D;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int P = Dp / PW;
  for (int pp = 0; pp < P; ++pp) {
    const int j0 = (UP ? pp : P - 1 - pp) * PW;
    const int col = j0 + lane;
    const bool colok = col < D;
    // diagonal tile: tile[j][i] = M[j0 + j][j0 + i] on the triangle this solve uses, the identity
    // on the padding
    for (int j = wid; j < PW; j += NW) {
      const bool tri = UP ? (UNIT ? j < lane : j <= lane) : (UNIT ? j > lane : j >= lane);
      float v = j == lane ? 1.f : 0.f;
      if (tri && colok && j0 + j < D) v = a.M[(long)(j0 + j) * a.ldm + col];
      tile[j * PW + lane] = v;
    }
    // off-panel dot products over the unknowns already solved
    {
      const int kbeg = UP ? 0 : j0 + PW, kend = UP ? j0 : Dp;
      float acc[R];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = 0.f;
#pragma unroll 2
      for (int kb = kbeg + 4 * wid; kb < kend; kb += 4 * NW) {
        float m[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          m[u] = (colok && kb + u < D) ? a.M[(long)(kb + u) * a.ldm + col] : 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float4 z = *reinterpret_cast<const float4*>(xs + r * Dp + kb);
          acc[r] = fmaf(m[0], z.x, acc[r]);
          acc[r] = fmaf(m[1], z.y, acc[r]);
          acc[r] = fmaf(m[2], z.z, acc[r]);
          acc[r] = fmaf(m[3], z.w, acc[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) part[(wid * R + r) * PW + lane] = acc[r];
    }
    __syncthreads();
    // in-panel substitution: lane = equation, 64 dependent steps
    {
      float rhs[RW];
#pragma unroll
      for (int q = 0; q < RW; ++q) {
        const int r = wid + NW * q;
        rhs[q] = 0.f;
        if (r < R) {
          const float p0 = part[(0 * R + r) * PW + lane], p1 = part[(1 * R + r) * PW + lane];
          const float p2 = part[(2 * R + r) * PW + lane], p3 = part[(3 * R + r) * PW + lane];
          rhs[q] = xs[r * Dp + col] - ((p0 + p1) + (p2 + p3));
        }
      }
      const float dg = UNIT ? 1.f : tile[lane * PW + lane];
#pragma unroll 4
      for (int jj = 0; jj < PW; ++jj) {
        const int j = UP ? jj : PW - 1 - jj;
        const float t = tile[j * PW + lane];
        const bool below = UP ? lane > j : lane < j;
        float dj = 1.f;
        if (!UNIT) dj = lane_value(dg, j);
#pragma unroll
        for (int q = 0; q < RW; ++q) {
          float xj = lane_value(rhs[q], j);
          if (!UNIT) xj = xj / dj;
          rhs[q] = lane == j ? xj : (below ? fmaf(-t, xj, rhs[q]) : rhs[q]);
        }
      }
#pragma unroll
      for (int q = 0; q < RW; ++q) {
        const int r = wid + NW * q;
        if (r < R) xs[r * Dp + col] = colok ? rhs[q] : 0.f;
      }
    }
    __syncthreads();
  }
}

template <int R>
__global__ __launch_bounds__(NT) void lu_solve_kernel(const LuArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int D = a.D, Dp = padded(D);
  float* xs = lds;                       // [R][Dp]
  float* part = xs + (long)R * Dp;       // [NW][R][PW] wave partials
  float* tile = part + NW * R * PW;      // [PW][PW] diagonal tile
  const int tid = threadIdx.x;
  const long row0 = (long)blockIdx.x * R;

  // stage: rows past the batch and the padding run on zeros and are never stored
  for (int r = 0; r < R; ++r) {
    const long row = row0 + r;
    for (int i = D + tid; i < Dp; i += NT) xs[r * Dp + i] = 0.f;
    for (int i = tid; i < D; i += NT) {
      float v = 0.f;
      if (row < a.B) {
        v = a.y[row * a.ldy + i];
        if (!a.transpose && a.bias != nullptr) v -= a.bias[i];
      }
      int dst = i;
      if (!a.transpose && a.perm != nullptr) dst = min(max(a.perm[i], 0), D - 1);
      xs[r * Dp + dst] = v;
    }
  }
  __syncthreads();

  if (a.mode == 0) {
    if (!a.transpose) {
      tri_solve<R, true, true>(a, xs, part, tile, Dp);     // L z = s
      tri_solve<R, false, false>(a, xs, part, tile, Dp);   // U x = z
    } else {
      tri_solve<R, true, false>(a, xs, part, tile, Dp);    // U^T q = gx
      tri_solve<R, false, true>(a, xs, part, tile, Dp);    // L^T g = q
    }
  } else if (!a.transpose) {
    tri_solve<R, true, false>(a, xs, part, tile, Dp);      // T x = s
  } else {
    tri_solve<R, false, false>(a, xs, part, tile, Dp);     // T^T g = gx
  }

  for (int r = 0; r < R; ++r) {
    const long row = row0 + r;
    if (row >= a.B) break;
    for (int i = tid; i < D; i += NT) {
      int src = i;
      if (a.transpose && a.perm != nullptr) src = min(max(a.perm[i], 0), D - 1);
      a.x[row * a.ldx + i] = xs[r * Dp + src];
    }
  }
}

template <int R>
void launch(const LuArgs& a, hipStream_t stream) {
  const size_t bytes = sizeof(float) * lds_floats(R, a.D);
  static bool attr_set = false;
  if (!attr_set) {
    NF_HIP_CHECK(hipFuncSetAttribute((const void*)lu_solve_kernel<R>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));
    attr_set = true;
  }
  const long blocks = ((long)a.B + R - 1) / R;
  hipLaunchKernelGGL(lu_solve_kernel<R>, dim3((unsigned)blocks), dim3(NT), bytes, stream, a);
  NF_HIP_CHECK(hipGetLastError());
}

}  // namespace

int nf_lu_solve_rows(int D) {
  if (D < 1 || D > kMaxD) return 0;
  for (int R = kMaxRows; R >= 1; R >>= 1)
    if (sizeof(float) * lds_floats(R, D) <= (size_t)kLdsBudget) return R;
  return 0;
}

void nf_launch_lu_solve(const NfLuSolve& s, hipStream_t stream) {
  LuArgs a{};
  a.M = s.M; a.ldm = s.ldm; a.y = s.y; a.ldy = s.ldy; a.perm = s.perm; a.bias = s.bias;
  a.x = s.x; a.ldx = s.ldx; a.B = s.B; a.D = s.D; a.mode = s.mode; a.transpose = s.transpose;
  switch (nf_lu_solve_rows(s.D)) {
    case 16: launch<16>(a, stream); break;
    case 8: launch<8>(a, stream); break;
    case 4: launch<4>(a, stream); break;
    case 2: launch<2>(a, stream); break;
    case 1: launch<1>(a, stream); break;
    default:
      nf_throw_hip_error(hipErrorInvalidValue, "lu_solve: D outside the kernel's limits",
                         __FILE__, __LINE__);
  }
}
