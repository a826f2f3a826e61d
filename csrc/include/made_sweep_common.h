// Shared frame of the degree-sweep kernels (made_sweep.hip: MAF sampling / IAF inverse with two
// outputs per coordinate; dsf_sweep.hip: the DSF inverse with 3U outputs and a root solve;
// rqs_sweep.hip: the spline inverse with 3K - 1 outputs and a closed-form transform): the
// kernel arguments, the block geometry and the LDS budget. The staging of a row tile, the
// hidden-unit phase of one step and the final store are the body fragments of
// made_sweep_phases.h; a kernel supplies the output phase and the transform of the coordinate of
// degree t between two barriers.
#pragma once

#include "nf_common.h"

namespace nf_sweep {

constexpr int NT = 256;          // threads per block (4 waves)
constexpr int NW = NT / 64;
constexpr int kLdsBudget = 81920;  // bytes per block: two blocks stay resident on a 160 KiB CU
// Rows per block: the largest power of two <= kMaxRows whose state fits kLdsBudget. A step is a
// chain of dependent waits (weights, LDS, shuffles, three barriers) that one block cannot fill, so
// blocks sharing a CU matter more than weight reuse: at (B, D, H) = (4096, 256, 512) a launch took
// 2.24 / 1.35 / 1.03 / 1.27 ms with 16 / 8 / 4 / 2 rows (docs/PERF_NOTES.md, "Degree sweep").
constexpr int kMaxRows = 8;

struct SweepArgs {
  const float* W[NF_MADE_SWEEP_MAX_HIDDEN];
  const float* b[NF_MADE_SWEEP_MAX_HIDDEN];
  long ldw[NF_MADE_SWEEP_MAX_HIDDEN];
  const float* Wo; long ldo;
  const float* bo;
  const float* v; long ldv;
  const float* ctx; long ldc;     // [B, H] added to layer 1's pre-activation, or null
  const int* perm;                // [D]: coordinate of degree t is perm[t - 1]
  const int* ubeg;                // [L, D + 2]: ubeg[l][t] = #{k : deg_l[k] < t}
  float* x; long ldx;
  float* ldj;
  int B, D, H, L, kind;
  float p;                        // bound (maf_sample) | gate_bias (iaf_gated) | scale (iaf_affine)
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

}  // namespace nf_sweep
