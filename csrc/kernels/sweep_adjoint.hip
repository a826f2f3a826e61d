// Adjoint degree sweep: the implicit gradient of the one-pass solves of made_sweep.hip,
// dsf_sweep.hip and rqs_sweep.hip, agnostic of the transform.
//
// The forward sweeps solve T(x) = v for a map that is triangular in degree order,
// v_i = tau(x_i; p_i), p_i = MADE_i(x_{<i}) in R^P. With d = dtau/dx, q = dtau/dp and the
// cotangents folded into gx = xbar - lbar dlog d/dx and c = lbar dlog d/dp, the cotangent w of v
// and pbar of p solve the TRANSPOSE of the forward substitution. Walking t = D .. 1 with
// i = perm[t - 1]:
//   1. the hidden units of degree t, layers L .. 1: their cotangents are complete, so
//      a_l[u] = hbar_l[u] [h_l[u] > 0] and it is pushed down: hbar_{l-1}[:n] += a_l[u] W_l[u, :n]
//      (l = 1: into xhat[:t], in degree order);
//   2. w_i = (gx_i - xhat_t) / d_i;  3. pbar_i = q_i w_i + c_i;
//   4. hbar_L[:c(t)] += sum_k pbar_{i,k} Wo[k D + i, :c(t)].
// Every in-mask weight is used once per row, and the prefixes written are the ones the forward
// sweep reads; entries outside the masks are never touched, so the weights need not be masked.
//
// Mapping: the frame of made_sweep_common.h - 256 threads own a tile of R rows whose state lives
// in LDS in fp32: xhat [R][D] in degree order, hbar_l [L][R][H] (overwritten by a_l) and the
// step's pbar [R][P]. Steps 1 and 4 give every thread one destination column: it adds the few
// units of degree t (or the P planes) one after the other in index order, reading weight rows
// coalesced, for all R rows. So there are no butterflies, no transposed weight copies and no
// atomics, and a row's sums depend only on (t, column): a row's result is bitwise the same for any
// R, any place in the tile and any batch. Rows past the batch run on zeros and are never stored.
// fp32 with explicit fmaf and an IEEE division.
#include "made_sweep_common.h"
#include "launchers.h"

namespace {

using namespace nf_sweep;

__host__ __device__ inline long adjoint_lds_floats(int R, int D, int H, int L, int P) {
  return (long)R * ((long)D + (long)L * H + P) + D;
}

template <int R>
__global__ __launch_bounds__(NT) void sweep_adjoint_kernel(const NfSweepAdjoint a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int D = a.D, H = a.H, L = a.L, P = a.P;
  float* xs = lds;                          // [R][D] xhat, degree order
  float* hs = xs + (long)R * D;             // [L][R][H] hbar_l, then a_l
  float* ps = hs + (long)L * R * H;         // [R][P] pbar of the step
  int* pl = reinterpret_cast<int*>(ps + (long)R * P);   // [D] perm
  const int tid = threadIdx.x;
  const long row0 = (long)blockIdx.x * R;
  const int W2 = D + 2;

  for (int p = tid; p < D; p += NT) pl[p] = clampi(a.perm[p], 0, D - 1);
  for (long k = tid; k < (long)R * ((long)D + (long)L * H); k += NT) lds[k] = 0.f;
  __syncthreads();

  float* hL = hs + (long)(L - 1) * R * H;
  for (int t = D; t >= 1; --t) {
    const int i = pl[t - 1];
    // ---- 1. hidden units of degree t, top layer first
    for (int l = L - 1; l >= 0; --l) {
      const int u0 = clampi(a.ubeg[l * W2 + t], 0, H);
      const int u1 = clampi(a.ubeg[l * W2 + t + 1], u0, H);
      if (u1 == u0) continue;   // block-uniform
      const int nu = u1 - u0;
      float* hl = hs + (long)l * R * H;
      for (int e = tid; e < R * nu; e += NT) {
        const int r = e / nu, u = u0 + (e - r * nu);
        const long row = row0 + r;
        const bool on = row < a.B && a.h[l][row * a.ldh[l] + u] > 0.f;
        const float av = on ? hl[r * H + u] : 0.f;
        hl[r * H + u] = av;
        if (row < a.B) a.a[l][row * a.lda[l] + u] = av;
      }
      __syncthreads();
      const int n = l == 0 ? t : clampi(a.ubeg[(l - 1) * W2 + t + 1], 0, H);
      float* dst = l == 0 ? xs : hs + (long)(l - 1) * R * H;
      const int ldt = l == 0 ? D : H;
      for (int j = tid; j < n; j += NT) {
        const float* wc = a.W[l] + (l == 0 ? pl[j] : j);
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = dst[r * ldt + j];
#pragma unroll 2
        for (int u = u0; u < u1; ++u) {
          const float wv = wc[(long)u * a.ldw[l]];
#pragma unroll
          for (int r = 0; r < R; ++r) acc[r] = fmaf(hl[r * H + u], wv, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) dst[r * ldt + j] = acc[r];
      }
      __syncthreads();
    }
    // ---- 2, 3. w and pbar of coordinate i (every thread of a row recomputes the same w)
    for (int e = tid; e < R * P; e += NT) {
      const int r = e / P, k = e - r * P;
      const long row = row0 + r;
      float pv = 0.f;
      if (row < a.B) {
        const float w = (a.gx[row * a.ldg + i] - xs[r * D + t - 1]) / a.d[row * a.ldd + i];
        const long off = (row * D + i) * P + k;
        pv = fmaf(a.q[off], w, a.c[off]);
        a.pbar[off] = pv;
        if (k == 0) a.w[row * a.ldwo + i] = w;
      }
      ps[r * P + k] = pv;
    }
    __syncthreads();
    // ---- 4. push pbar into the prefix of the last hidden layer
    const int c = clampi(a.ubeg[(L - 1) * W2 + t], 0, H);
    for (int j = tid; j < c; j += NT) {
      const float* wc = a.Wo + (long)i * a.ldo + j;
      float acc[R];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = hL[r * H + j];
#pragma unroll 2
      for (int k = 0; k < P; ++k) {
        const float wv = wc[(long)k * D * a.ldo];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fmaf(ps[r * P + k], wv, acc[r]);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) hL[r * H + j] = acc[r];
    }
    __syncthreads();
  }
}

template <int R>
void launch(const NfSweepAdjoint& a, hipStream_t stream) {
  const size_t bytes = sizeof(float) * adjoint_lds_floats(R, a.D, a.H, a.L, a.P);
  static bool attr_set = false;
  if (!attr_set) {
    NF_HIP_CHECK(hipFuncSetAttribute((const void*)sweep_adjoint_kernel<R>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));
    attr_set = true;
  }
  const long blocks = ((long)a.B + R - 1) / R;
  hipLaunchKernelGGL(sweep_adjoint_kernel<R>, dim3((unsigned)blocks), dim3(NT), bytes, stream, a);
  NF_HIP_CHECK(hipGetLastError());
}

}  // namespace

int nf_sweep_adjoint_rows(int D, int H, int L, int P) {
  if (D < 1 || H < 1 || L < 1 || L > NF_MADE_SWEEP_MAX_HIDDEN || P < 1 ||
      P > NF_SWEEP_ADJOINT_MAX_P)
    return 0;
  for (int R = kMaxRows; R >= 1; R >>= 1)
    if (sizeof(float) * adjoint_lds_floats(R, D, H, L, P) <= (size_t)kLdsBudget) return R;
  return 0;
}

void nf_launch_sweep_adjoint(const NfSweepAdjoint& s, hipStream_t stream) {
  switch (nf_sweep_adjoint_rows(s.D, s.H, s.L, s.P)) {
    case 8: launch<8>(s, stream); break;
    case 4: launch<4>(s, stream); break;
    case 2: launch<2>(s, stream); break;
    case 1: launch<1>(s, stream); break;
    default:
      nf_throw_hip_error(hipErrorInvalidValue, "sweep_adjoint: shape exceeds the LDS budget",
                         __FILE__, __LINE__);
  }
}
