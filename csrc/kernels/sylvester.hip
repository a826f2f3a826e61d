// Fused K-layer Sylvester flow stack (van den Berg et al. 2018), forward + backward (gfx950).
//
// Per layer k, state z in R^D (definition: ops/reference.py sylvester_stack_reference):
//   t  = H_H ... H_1 P^f z        H_h x = x - 2 v_h (v_h.x) / max(v_h.v_h, 1e-20), P = reversal
//   a  = d2 * t + R2 t + b        R1, R2 strictly upper triangular, packed by column:
//   h  = tanh(a)                  entry (i, j), i < j, at j (j - 1) / 2 + i
//   y  = d1 * h + R1 h
//   z' = z + P^f H_1 ... H_H y
//   ldj += sum_i log(|1 + (1 - h_i^2) d1_i d2_i| + 1e-7)
//
// One wave64 (one 64-thread block) per row, lane i owns coordinate i (D <= 64); the K-loop lives
// in the kernel, state and ldj stay in registers. Every parameter tensor is addressed as
// base + row * row_stride + k * width + index (inner [K, width] dense): row stride 0 is a shared
// parameter, and a column slice of an encoder output [N, Dout] is read in place.
//
// A layer's R1, R2 and V are staged through LDS with full-width coalesced loads issued together
// (the packed columns are short: a direct read of column j fills j of 64 lanes; and a reflection
// vector fetched where it is used puts one memory latency into each of the 2 H dependent steps).
// From LDS the forward mat-vec reads column j with adjacent lanes (conflict-free), and the
// backward's transposed mat-vec reads lane i's own column i, which in global memory would be a
// stride across lanes. The backward builds dR1 / dR2 in the same LDS image and writes them out
// full width. Nothing outside the strict upper part exists in the packed layout, so it is never
// touched.
//
// Backward of a layer, from its saved input: recompute t, a, h, y; gy = Q^T g is the forward
// chain applied to g; gh = d1 gy + R1^T gy + ldj term, ga = gh (1 - h^2), gt = d2 ga + R2^T ga;
// dz = g + Q gt. Reflections are involutions, so both chains are unwound from their far ends
// (t and y) one reflection at a time, giving each H_h's input and output gradient without
// storing the intermediate vectors; the two contributions to dV_h are added in registers.
#include "nf_common.h"

namespace nf {

constexpr float kSylEps = 1e-7f;     // the log|psi| guard of planar.hip
constexpr float kSylVvMin = 1e-20f;  // v = 0 is the identity reflection

__device__ __forceinline__ float syl_dlog_guard(float psi) {
  return copysignf(1.f / (fabsf(psi) + kSylEps), psi);
}

// value of lane j (wave-uniform j)
__device__ __forceinline__ float lane_bcast(float x, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j));
}

template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(
                 __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

// Sum over the wave, the same bits in every lane; all 64 lanes must be active. A layer is a
// chain of up to 2 H dependent dot products, so the latency of one reduction sets the time of a
// row: four DPP adds (lane ^ 1, lane ^ 2, mirror within 8, mirror within 16) leave each row of
// 16 lanes with its sum, and the four row sums are read as scalars - no LDS-crossbar shuffle.
__device__ __forceinline__ float syl_wave_sum(float v) {
  v = dpp_add<0xB1>(v);    // quad_perm [1, 0, 3, 2]
  v = dpp_add<0x4E>(v);    // quad_perm [2, 3, 0, 1]
  v = dpp_add<0x141>(v);   // row_half_mirror
  v = dpp_add<0x140>(v);   // row_mirror
  return (lane_bcast(v, 0) + lane_bcast(v, 16)) + (lane_bcast(v, 32) + lane_bcast(v, 48));
}

// coordinate reversal on lanes < D (lanes >= D hold 0)
__device__ __forceinline__ float flip_lanes(float x, int lane, int D) {
  const float r = __shfl(x, lane < D ? D - 1 - lane : lane, 64);
  return lane < D ? r : 0.f;
}

// Copy n floats of one or two global arrays into LDS, 8 full-width loads per array in flight
// before the first store (a plain copy loop waits for each load in turn, and at one wave per
// SIMD the layer then costs a memory latency per 64 floats).
__device__ __forceinline__ void stage2(float* la, const float* ga, float* lb, const float* gb,
                                       int n, int lane) {
  for (int i0 = lane; i0 < n; i0 += 512) {
    float ra[8], rb[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + 64 * u;
      ra[u] = i < n ? ga[i] : 0.f;
      rb[u] = (gb && i < n) ? gb[i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + 64 * u;
      if (i < n) {
        la[i] = ra[u];
        if (gb) lb[i] = rb[u];
      }
    }
  }
}

// sum_{j > i} R[i, j] x_j for lane i; Rl = LDS image of the packed R
__device__ __forceinline__ float mv_upper(const float* Rl, float x, int lane, int D) {
  float acc = 0.f;
#pragma unroll 4
  for (int j = 1; j < D; ++j) {
    const float xj = lane_bcast(x, j);
    const bool in = lane < j;                       // no branch: the reads of several columns
    const float r = Rl[in ? j * (j - 1) / 2 + lane : 0];   // are in flight together
    acc += in ? r * xj : 0.f;
  }
  return acc;
}

// sum_{j < i} R[j, i] x_j for lane i (R^T x): lane i walks its own column
__device__ __forceinline__ float mv_upper_t(const float* Rl, float x, int lane, int D) {
  float acc = 0.f;
  const int col = lane * (lane - 1) / 2;
#pragma unroll 4
  for (int j = 0; j + 1 < D; ++j) {
    const float xj = lane_bcast(x, j);
    const bool in = j < lane && lane < D;
    const float r = Rl[in ? col + j : 0];
    acc += in ? r * xj : 0.f;
  }
  return acc;
}

// LDS image of the outer product o[i, j] = p_i q_j, i < j, packed
__device__ __forceinline__ void outer_upper(float* Rl, float p, float q, int lane, int D) {
  for (int j = 1; j < D; ++j) {
    const float qj = lane_bcast(q, j);
    if (lane < j) Rl[j * (j - 1) / 2 + lane] = p * qj;
  }
}

struct SylArgs {
  NfSylParams p;
  NfSylGrads g;
  const float* z;       // [N, D]
  float* zK;            // [N, D]
  float* ldj;           // [N]
  float* saved;         // [N, K, D] layer inputs (forward: written, backward: read)
  const float* gz;      // [N, D]
  const float* gl;      // [N]
  float* dz;            // [N, D]
  unsigned long long flipmask;  // bit i: layer k0 + i reverses the coordinates
  int N, D, K, H;
  int k0, kn;           // this launch runs layers [k0, k0 + kn), kn <= 64
  int ldj_acc;          // forward: add to ldj instead of initialising it
};

__global__ void __launch_bounds__(64) sylvester_fwd_kernel(SylArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x;
  const long row = blockIdx.x;
  const int D = a.D, H = a.H, P = D * (D - 1) / 2;
  const bool on = lane < D;
  float* R1l = lds;
  float* R2l = lds + P;
  float* Vl = lds + 2 * P;   // [H][D]
  float z = on ? a.z[row * D + lane] : 0.f;
  float ldj = 0.f;
  for (int kk = 0; kk < a.kn; ++kk) {
    const int k = a.k0 + kk;
    const bool flip = (a.flipmask >> kk) & 1ull;
    if (a.saved && on) a.saved[(row * a.K + k) * D + lane] = z;
    const float* r1 = a.p.R1 + row * a.p.rs_R1 + (long)k * P;
    const float* r2 = a.p.R2 + row * a.p.rs_R2 + (long)k * P;
    const float* vk = a.p.V + row * a.p.rs_V + (long)k * H * D;
    __syncthreads();
    stage2(R1l, r1, R2l, r2, P, lane);
    stage2(Vl, vk, nullptr, nullptr, H * D, lane);
    __syncthreads();
    const long pv = row * a.p.rs_d1 + (long)k * D + lane;
    const float d1 = on ? a.p.d1[pv] : 0.f;
    const float d2 = on ? a.p.d2[row * a.p.rs_d2 + (long)k * D + lane] : 0.f;
    const float b = on ? a.p.b[row * a.p.rs_b + (long)k * D + lane] : 0.f;
    float t = flip ? flip_lanes(z, lane, D) : z;
    for (int h = 0; h < H; ++h) {
      const float v = on ? Vl[h * D + lane] : 0.f;
      const float inv2 = 2.f / fmaxf(syl_wave_sum(v * v), kSylVvMin);
      t -= v * (syl_wave_sum(v * t) * inv2);
    }
    const float hv = tanhf(d2 * t + mv_upper(R2l, t, lane, D) + b);
    float y = d1 * hv + mv_upper(R1l, hv, lane, D);
    for (int h = H - 1; h >= 0; --h) {
      const float v = on ? Vl[h * D + lane] : 0.f;
      const float inv2 = 2.f / fmaxf(syl_wave_sum(v * v), kSylVvMin);
      y -= v * (syl_wave_sum(v * y) * inv2);
    }
    z += flip ? flip_lanes(y, lane, D) : y;
    if (on) ldj += logf(fabsf(1.f + (1.f - hv * hv) * d1 * d2) + kSylEps);
  }
  if (on) a.zK[row * D + lane] = z;
  ldj = syl_wave_sum(ldj);
  if (lane == 0) a.ldj[row] = a.ldj_acc ? a.ldj[row] + ldj : ldj;
}

__global__ void __launch_bounds__(64) sylvester_bwd_kernel(SylArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x;
  const long row = blockIdx.x;
  const int D = a.D, H = a.H, P = D * (D - 1) / 2;
  const bool on = lane < D;
  float* R1l = lds;
  float* R2l = lds + P;
  float* Vl = lds + 2 * P;   // [H][D]
  float g = on ? a.gz[row * D + lane] : 0.f;
  const float c = a.gl[row];
  for (int kk = a.kn - 1; kk >= 0; --kk) {
    const int k = a.k0 + kk;
    const bool flip = (a.flipmask >> kk) & 1ull;
    const float z = on ? a.saved[(row * a.K + k) * D + lane] : 0.f;
    const float* r1 = a.p.R1 + row * a.p.rs_R1 + (long)k * P;
    const float* r2 = a.p.R2 + row * a.p.rs_R2 + (long)k * P;
    const float* vk = a.p.V + row * a.p.rs_V + (long)k * H * D;
    __syncthreads();
    stage2(R1l, r1, R2l, r2, P, lane);
    stage2(Vl, vk, nullptr, nullptr, H * D, lane);
    __syncthreads();
    const float d1 = on ? a.p.d1[row * a.p.rs_d1 + (long)k * D + lane] : 0.f;
    const float d2 = on ? a.p.d2[row * a.p.rs_d2 + (long)k * D + lane] : 0.f;
    const float b = on ? a.p.b[row * a.p.rs_b + (long)k * D + lane] : 0.f;
    // recompute t, h, y and push g through the same chain: gy = Q^T g
    float t = flip ? flip_lanes(z, lane, D) : z;
    float gy = flip ? flip_lanes(g, lane, D) : g;
    for (int h = 0; h < H; ++h) {
      const float v = on ? Vl[h * D + lane] : 0.f;
      const float inv2 = 2.f / fmaxf(syl_wave_sum(v * v), kSylVvMin);
      t -= v * (syl_wave_sum(v * t) * inv2);
      gy -= v * (syl_wave_sum(v * gy) * inv2);
    }
    const float hv = tanhf(d2 * t + mv_upper(R2l, t, lane, D) + b);
    const float hp = 1.f - hv * hv;
    const float y = d1 * hv + mv_upper(R1l, hv, lane, D);
    const float q = on ? c * syl_dlog_guard(1.f + hp * d1 * d2) : 0.f;   // dL / dpsi_i
    const float gh = d1 * gy + mv_upper_t(R1l, gy, lane, D) - 2.f * q * hv * d1 * d2;
    const float ga = gh * hp;
    const float gt = d2 * ga + mv_upper_t(R2l, ga, lane, D);
    const long go = (long)k * D + lane;
    if (on) {
      a.g.d1[row * a.g.rs_d1 + go] = gy * hv + q * hp * d2;
      a.g.d2[row * a.g.rs_d2 + go] = ga * t + q * hp * d1;
      a.g.b[row * a.g.rs_b + go] = ga;
    }
    // dR1[i, j] = gy_i h_j, dR2[i, j] = ga_i t_j, built over the staged R and written full width
    __syncthreads();
    outer_upper(R1l, gy, hv, lane, D);
    outer_upper(R2l, ga, t, lane, D);
    __syncthreads();
    float* o1 = a.g.R1 + row * a.g.rs_R1 + (long)k * P;
    float* o2 = a.g.R2 + row * a.g.rs_R2 + (long)k * P;
    for (int i = lane; i < P; i += 64) {
      o1[i] = R1l[i];
      o2[i] = R2l[i];
    }
    // unwind both chains from their far ends. Chain A (t = H_H .. H_1 x0): xa is H_h's output,
    // ra its gradient. Chain B (u = H_1 .. H_H y): yb is H_h's input, rb its input gradient.
    float xa = t, ra = gt, yb = y, rb = gy;
    float* dv = a.g.V + row * a.g.rs_V + (long)k * H * D + lane;
    for (int h = H - 1; h >= 0; --h) {
      const float v = on ? Vl[h * D + lane] : 0.f;
      const float vv = syl_wave_sum(v * v);
      const float inv = 1.f / fmaxf(vv, kSylVvMin);
      const float live = vv >= kSylVvMin ? 1.f : 0.f;   // the clamp passes no gradient below it
      const float keep = 1.f - 2.f * vv * inv;          // v.(H x) = keep * v.x
      // A: input xin = H_h xa; r = H_h(xin), gradient ra w.r.t. r
      const float sa_out = syl_wave_sum(v * xa);
      const float pa = syl_wave_sum(v * ra);
      const float xin = xa - v * (2.f * sa_out * inv);
      const float sa = sa_out * keep;                   // v.xin
      float gv = -2.f * inv * (sa * ra + pa * xin) + live * 4.f * sa * pa * inv * inv * v;
      ra -= v * (2.f * pa * inv);
      xa = xin;
      // B: input yb, output gradient rout = H_h rb
      const float sb = syl_wave_sum(v * yb);
      const float pb_in = syl_wave_sum(v * rb);
      const float rout = rb - v * (2.f * pb_in * inv);
      const float pb = pb_in * keep;                    // v.rout
      gv += -2.f * inv * (sb * rout + pb * yb) + live * 4.f * sb * pb * inv * inv * v;
      yb -= v * (2.f * sb * inv);
      rb = rout;
      if (on) dv[h * D] = gv;
    }
    g += flip ? flip_lanes(ra, lane, D) : ra;
  }
  if (on) a.dz[row * D + lane] = g;
}

static size_t syl_lds_bytes(int D, int H) {
  const size_t n = (size_t)D * (D - 1) + (size_t)H * D;   // R1, R2, V of one layer
  return (n > 1 ? n : 1) * sizeof(float);
}

// layers in launches of <= 64 (one flip bit each); a later forward launch continues from zK /
// ldj in place, an earlier backward launch from dz in place (a row is read before it is written
// and belongs to one wave)
static void syl_run(SylArgs a, const unsigned char* flips, bool bwd, hipStream_t stream) {
  const int K = a.K;
  const int nseg = (K + 63) / 64;
  for (int s = 0; s < nseg; ++s) {
    const int seg = bwd ? nseg - 1 - s : s;
    a.k0 = seg * 64;
    a.kn = K - a.k0 < 64 ? K - a.k0 : 64;
    a.flipmask = 0;
    for (int i = 0; i < a.kn; ++i)
      if (flips[a.k0 + i]) a.flipmask |= 1ull << i;
    if (s > 0) {
      if (bwd) {
        a.gz = a.dz;
      } else {
        a.z = a.zK;
        a.ldj_acc = 1;
      }
    }
    const dim3 grid((unsigned)a.N), block(64);
    const size_t lds = syl_lds_bytes(a.D, a.H);
    if (bwd)
      hipLaunchKernelGGL(sylvester_bwd_kernel, grid, block, lds, stream, a);
    else
      hipLaunchKernelGGL(sylvester_fwd_kernel, grid, block, lds, stream, a);
    NF_HIP_CHECK(hipGetLastError());
  }
}

}  // namespace nf

using namespace nf;

void nf_launch_sylvester_fwd(const float* z, const NfSylParams& p, const unsigned char* flips,
                             float* zK, float* ldj, float* saved, int N, int D, int K, int H,
                             hipStream_t stream) {
  if (N <= 0 || K <= 0) return;
  SylArgs a{};
  a.p = p; a.z = z; a.zK = zK; a.ldj = ldj; a.saved = saved;
  a.N = N; a.D = D; a.K = K; a.H = H;
  syl_run(a, flips, false, stream);
}

void nf_launch_sylvester_bwd(const float* saved, const NfSylParams& p, const unsigned char* flips,
                             const float* gz, const float* gl, float* dz, const NfSylGrads& g,
                             int N, int D, int K, int H, hipStream_t stream) {
  if (N <= 0 || K <= 0) return;
  SylArgs a{};
  a.p = p; a.g = g; a.saved = (float*)saved; a.gz = gz; a.gl = gl; a.dz = dz;
  a.N = N; a.D = D; a.K = K; a.H = H;
  syl_run(a, flips, true, stream);
}
