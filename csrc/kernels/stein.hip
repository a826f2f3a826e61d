// All-pairs Stein kernels: the SVGD direction and the rows of the Stein kernel matrix (KSD).
//
//   phi_i  = (1/N) sum_j [ f_ij s_j - 2 f'_ij (x_i - x_j) ]
//   u_ij   = f (s_i . s_j) + 2 f' (s_j - s_i) . (x_i - x_j) - 2 D f' - 4 f'' r2
//   rows_i = sum_j u_ij,  diag_i = u_ii
//
// with f a function of r2 = |x_i - x_j|^2 and one bandwidth h: "rbf" f = exp(-r2 / h), "imq"
// f = (h + r2)^(-1/2). fp32, 1 <= D <= 64; neither N x N matrix is ever stored.
//
// A workgroup owns NF_STEIN_TILE_I rows i. Row i lives in registers (x_i, s_i and the
// accumulators), split over LPR adjacent lanes of C coordinates each for D > 16 (C = 16, LPR = 2
// or 4) so that no lane carries more than 3 x 16 row values; r2 and the two dot products are then
// completed with LPR-wide xor shuffles. r2 is summed from the differences x_i - x_j themselves:
// |x_i|^2 + |x_j|^2 - 2 x_i . x_j cancels exactly where the kernel weight is largest. Tiles of
// NF_STEIN_TILE_J rows j are staged in LDS as [x_j | s_j], zero-padded to the compile-time
// width C LPR; every lane of a part reads the same j, a broadcast read.
//
// The grid is (i-tiles, j_splits): split s takes the j-tiles [s T / S, (s + 1) T / S) and writes
// its partial sums to work[s]; a second kernel adds the partials in the order s = 0 .. S - 1.
// No atomics anywhere, so a result is bitwise repeatable for a given (N, D, j_splits).
#include "nf_common.h"
#include "stein_tiles.h"

namespace nf {
namespace {

constexpr int TI = NF_STEIN_TILE_I;
constexpr int TJ = NF_STEIN_TILE_J;
constexpr int KIND_RBF = 0, KIND_IMQ = 1;

struct SteinArgs {
  const float* x;
  const float* s;
  long ldx, lds;       // row strides in elements (unit inner stride)
  const float* h_dev;  // 1-element device bandwidth, or null -> h_host
  float h_host;
  float* work;         // [S, N, D] (svgd) or [S, N] (ksd)
  float* diag;         // ksd only
  int N, D, S;
};

// f, f' and f'' of r2 for the two kernel functions
template <int KIND>
struct KFun;

template <>
struct KFun<KIND_RBF> {
  float inv_h, nl2e_h;
  __device__ explicit KFun(float h) : inv_h(1.f / h), nl2e_h(-1.4426950408889634f / h) {}
  __device__ __forceinline__ void eval(float r2, float& f, float& fp) const {
    f = __builtin_amdgcn_exp2f(r2 * nl2e_h);   // v_exp_f32: e^(-r2 / h)
    fp = -f * inv_h;
  }
  __device__ __forceinline__ void eval2(float r2, float& f, float& fp, float& fpp) const {
    eval(r2, f, fp);
    fpp = -fp * inv_h;
  }
};

template <>
struct KFun<KIND_IMQ> {
  float h;
  __device__ explicit KFun(float h_) : h(h_) {}
  __device__ __forceinline__ void eval(float r2, float& f, float& fp) const {
    f = rsqrtf(h + r2);
    fp = -0.5f * f * (f * f);
  }
  __device__ __forceinline__ void eval2(float r2, float& f, float& fp, float& fpp) const {
    eval(r2, f, fp);
    fpp = -1.5f * fp * (f * f);
  }
};

// sum over the LPR adjacent lanes that share a row; every one of them gets the same bits
template <int LPR>
__device__ __forceinline__ float part_sum(float v) {
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// rows [j0, j0 + TJ) of x and s -> tile[j][x (DP) | s (DP)], zero beyond N and beyond D
template <int DP, int NT>
__device__ __forceinline__ void stage_tile(const SteinArgs& a, long j0, float* tile) {
  for (int idx = threadIdx.x; idx < TJ * DP; idx += NT) {
    const int j = idx / DP, c = idx % DP;
    const long gj = j0 + j;
    const bool ok = gj < a.N && c < a.D;
    tile[j * 2 * DP + c] = ok ? a.x[gj * a.ldx + c] : 0.f;
    tile[j * 2 * DP + DP + c] = ok ? a.s[gj * a.lds + c] : 0.f;
  }
}

template <int C, int LPR, int KIND>
__global__ __launch_bounds__(TI* LPR) void stein_svgd_kernel(SteinArgs a) {
  constexpr int DP = C * LPR, NT = TI * LPR;
  __shared__ __align__(16) float tile[TJ * 2 * DP];
  const int part = threadIdx.x % LPR, row = threadIdx.x / LPR;
  const long i = (long)blockIdx.x * TI + row;
  const int split = blockIdx.y;
  const KFun<KIND> kf(a.h_dev ? *a.h_dev : a.h_host);

  float xi[C], acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int gc = part * C + c;
    xi[c] = (i < a.N && gc < a.D) ? a.x[i * a.ldx + gc] : 0.f;
    acc[c] = 0.f;
  }

  const long nt = ((long)a.N + TJ - 1) / TJ;
  const long t0 = split * nt / a.S, t1 = (split + 1) * nt / a.S;
  for (long t = t0; t < t1; ++t) {
    const long j0 = t * TJ;
    const int jn = (int)(a.N - j0 < TJ ? a.N - j0 : TJ);
    __syncthreads();
    stage_tile<DP, NT>(a, j0, tile);
    __syncthreads();
#pragma unroll 2
    for (int j = 0; j < jn; ++j) {
      const float* tj = tile + j * 2 * DP + part * C;
      float d[C], r2 = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        d[c] = xi[c] - tj[c];
        r2 = fmaf(d[c], d[c], r2);
      }
      r2 = part_sum<LPR>(r2);
      float f, fp;
      kf.eval(r2, f, fp);
      const float w = -2.f * fp;
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = fmaf(w, d[c], fmaf(f, tj[DP + c], acc[c]));
    }
  }

  if (i < a.N) {
    float* out = a.work + ((long)split * a.N + i) * a.D;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int gc = part * C + c;
      if (gc < a.D) out[gc] = acc[c];
    }
  }
}

template <int C, int LPR, int KIND>
__global__ __launch_bounds__(TI* LPR) void stein_ksd_kernel(SteinArgs a) {
  constexpr int DP = C * LPR, NT = TI * LPR;
  __shared__ __align__(16) float tile[TJ * 2 * DP];
  const int part = threadIdx.x % LPR, row = threadIdx.x / LPR;
  const long i = (long)blockIdx.x * TI + row;
  const int split = blockIdx.y;
  const KFun<KIND> kf(a.h_dev ? *a.h_dev : a.h_host);
  const float two_d = 2.f * (float)a.D;

  float xi[C], si[C], sii = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int gc = part * C + c;
    const bool ok = i < a.N && gc < a.D;
    xi[c] = ok ? a.x[i * a.ldx + gc] : 0.f;
    si[c] = ok ? a.s[i * a.lds + gc] : 0.f;
    sii = fmaf(si[c], si[c], sii);
  }
  sii = part_sum<LPR>(sii);

  float usum = 0.f;
  const long nt = ((long)a.N + TJ - 1) / TJ;
  const long t0 = split * nt / a.S, t1 = (split + 1) * nt / a.S;
  for (long t = t0; t < t1; ++t) {
    const long j0 = t * TJ;
    const int jn = (int)(a.N - j0 < TJ ? a.N - j0 : TJ);
    __syncthreads();
    stage_tile<DP, NT>(a, j0, tile);
    __syncthreads();
#pragma unroll 2
    for (int j = 0; j < jn; ++j) {
      const float* tj = tile + j * 2 * DP + part * C;
      float r2 = 0.f, ss = 0.f, sd = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float d = xi[c] - tj[c], sj = tj[DP + c];
        r2 = fmaf(d, d, r2);
        ss = fmaf(si[c], sj, ss);
        sd = fmaf(sj - si[c], d, sd);
      }
      r2 = part_sum<LPR>(r2);
      ss = part_sum<LPR>(ss);
      sd = part_sum<LPR>(sd);
      float f, fp, fpp;
      kf.eval2(r2, f, fp, fpp);
      usum += fmaf(f, ss, 2.f * fp * sd) - fmaf(two_d, fp, 4.f * fpp * r2);
    }
  }

  if (i < a.N && part == 0) {
    a.work[(long)split * a.N + i] = usum;
    if (split == 0) {
      float f, fp, fpp;
      kf.eval2(0.f, f, fp, fpp);
      a.diag[i] = fmaf(f, sii, -two_d * fp);
    }
  }
}

// out[e] = (work[0][e] + work[1][e] + ... + work[S - 1][e]) / denom, in that order
__global__ __launch_bounds__(256) void stein_reduce_kernel(const float* __restrict__ work,
                                                           float* __restrict__ out, long n, int S,
                                                           float denom) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  float acc = 0.f;
  for (int s = 0; s < S; ++s) acc += work[(long)s * n + e];
  out[e] = acc / denom;
}

template <int C, int LPR>
void launch_pairs(const SteinArgs& a, int kind, bool ksd, hipStream_t stream) {
  const dim3 grid((unsigned)(((long)a.N + TI - 1) / TI), (unsigned)a.S), block(TI * LPR);
  if (ksd) {
    if (kind == KIND_RBF)
      hipLaunchKernelGGL((stein_ksd_kernel<C, LPR, KIND_RBF>), grid, block, 0, stream, a);
    else
      hipLaunchKernelGGL((stein_ksd_kernel<C, LPR, KIND_IMQ>), grid, block, 0, stream, a);
  } else {
    if (kind == KIND_RBF)
      hipLaunchKernelGGL((stein_svgd_kernel<C, LPR, KIND_RBF>), grid, block, 0, stream, a);
    else
      hipLaunchKernelGGL((stein_svgd_kernel<C, LPR, KIND_IMQ>), grid, block, 0, stream, a);
  }
  NF_HIP_CHECK(hipGetLastError());
}

void run_pairs(const SteinArgs& a, int kind, bool ksd, hipStream_t stream) {
  const int D = a.D;
  if (D <= 1) launch_pairs<1, 1>(a, kind, ksd, stream);
  else if (D <= 2) launch_pairs<2, 1>(a, kind, ksd, stream);
  else if (D <= 4) launch_pairs<4, 1>(a, kind, ksd, stream);
  else if (D <= 8) launch_pairs<8, 1>(a, kind, ksd, stream);
  else if (D <= 16) launch_pairs<16, 1>(a, kind, ksd, stream);
  else if (D <= 32) launch_pairs<16, 2>(a, kind, ksd, stream);
  else launch_pairs<16, 4>(a, kind, ksd, stream);
}

void run_reduce(const float* work, float* out, long n, int S, float denom, hipStream_t stream) {
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipLaunchKernelGGL(stein_reduce_kernel, grid, block, 0, stream, work, out, n, S, denom);
  NF_HIP_CHECK(hipGetLastError());
}

}  // namespace
}  // namespace nf

using namespace nf;

int nf_stein_splits(int N, int D, int j_splits) {
  (void)D;
  if (j_splits > 0) return j_splits;
  // enough workgroups for the whole card at small N, never more splits than j-tiles
  const long it = ((long)N + TI - 1) / TI, nt = ((long)N + TJ - 1) / TJ;
  long S = (1024 + it - 1) / (it > 0 ? it : 1);
  if (S > nt) S = nt;
  if (S > 64) S = 64;
  return S < 1 ? 1 : (int)S;
}

void nf_launch_stein_svgd(const float* x, long ldx, const float* score, long lds,
                          const float* h_dev, float h_host, int kind, int S, float* phi,
                          float* work, int N, int D, hipStream_t stream) {
  if (N <= 0) return;
  SteinArgs a{x, score, ldx, lds, h_dev, h_host, work, nullptr, N, D, S};
  run_pairs(a, kind, false, stream);
  run_reduce(work, phi, (long)N * D, S, (float)N, stream);
}

void nf_launch_stein_ksd(const float* x, long ldx, const float* score, long lds,
                         const float* h_dev, float h_host, int kind, int S, float* rows,
                         float* diag, float* work, int N, int D, hipStream_t stream) {
  if (N <= 0) return;
  SteinArgs a{x, score, ldx, lds, h_dev, h_host, work, diag, N, D, S};
  run_pairs(a, kind, true, stream);
  run_reduce(work, rows, (long)N, S, 1.f, stream);
}
