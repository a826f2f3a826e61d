// The phases the degree-sweep kernels run verbatim (made_sweep.hip, dsf_sweep.hip, rqs_sweep.hip).
// This file is
// a BODY FRAGMENT: it is included inside a kernel, once per phase, with NF_SWEEP_PHASE set to
//   1  stage:  clamped perm into LDS, then v in degree order and every hidden layer pre-filled
//              with bias (+ context projection); ends with a barrier
//   2  hidden: the hidden units of degree t, layer by layer: one wave per unit, lanes strided over
//              the inputs, wave butterfly; every non-empty layer ends with a barrier
//   3  store:  x back in coordinate order, for the rows inside the batch
// and uses the kernel's own names: a (nf_sweep::SweepArgs), R, D, H, L, W2 = D + 2, xs [R][D],
// hs [L][R][H], pl [D], tid, lane, wid, row0 and, for phase 2, t. It is text and not a function
// on purpose: as __forceinline__ functions the same statements compiled made_sweep_kernel to a
// different instruction stream that ran 1-2 % slower (docs/PERF_NOTES.md, "DSF degree sweep");
// included as text, made_sweep.hip compiles to exactly what it was before the phases were shared.
#if NF_SWEEP_PHASE == 1
  for (int p = tid; p < D; p += NT) pl[p] = clampi(a.perm[p], 0, D - 1);
  __syncthreads();
  // stage v in degree order; rows past the batch run on zeros and are never stored
  for (int r = 0; r < R; ++r) {
    const long row = row0 + r;
    for (int p = tid; p < D; p += NT)
      xs[r * D + p] = row < a.B ? a.v[row * a.ldv + pl[p]] : 0.f;
    for (int l = 0; l < L; ++l)
      for (int k = tid; k < H; k += NT) {
        float bv = a.b[l][k];
        if (l == 0 && a.ctx != nullptr && row < a.B) bv += a.ctx[row * a.ldc + k];
        hs[((long)l * R + r) * H + k] = bv;
      }
  }
  __syncthreads();
#elif NF_SWEEP_PHASE == 2
    for (int l = 0; l < L; ++l) {
      const int u0 = clampi(a.ubeg[l * W2 + t], 0, H);
      const int u1 = clampi(a.ubeg[l * W2 + t + 1], u0, H);
      if (u1 == u0) continue;   // block-uniform
      const int n = l == 0 ? t : clampi(a.ubeg[(l - 1) * W2 + t + 1], 0, H);
      const float* in = l == 0 ? xs : hs + (long)(l - 1) * R * H;
      const int ldi = l == 0 ? D : H;
      float* out = hs + (long)l * R * H;
      for (int k = u0 + wid; k < u1; k += NW) {
        const float* w = a.W[l] + (long)k * a.ldw[l];
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.f;
#pragma unroll 2
        for (int j = lane; j < n; j += 64) {
          const float wv = l == 0 ? w[pl[j]] : w[j];
#pragma unroll
          for (int r = 0; r < R; ++r) acc[r] = fmaf(wv, in[r * ldi + j], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float sum = nf::wave_sum(acc[r]);
          if (lane == r) out[r * H + k] = fmaxf(out[r * H + k] + sum, 0.f);
        }
      }
      __syncthreads();
    }
#elif NF_SWEEP_PHASE == 3
  for (int r = 0; r < R; ++r) {
    const long row = row0 + r;
    if (row >= a.B) break;
    for (int p = tid; p < D; p += NT) a.x[row * a.ldx + pl[p]] = xs[r * D + p];
  }
#else
#error "made_sweep_phases.h: set NF_SWEEP_PHASE to 1 (stage), 2 (hidden) or 3 (store)"
#endif
#undef NF_SWEEP_PHASE
