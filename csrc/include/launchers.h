// Host-side launcher declarations shared by csrc/kernels/*.hip and csrc/bindings/*.cpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

void nf_throw_hip_error(hipError_t e, const char* expr, const char* file, int line);

// coupling.hip
void nf_launch_coupling_fwd(const void* st, int st_is_bf16, long ld_st_, const float* x, long ld_x,
                            float* y, long ld_y, void* ybf, int ybf_is_bf16, long ld_yb,
                            float* ssav, long ld_s, float* ldj, int B, int Dh, float scale,
                            int inverse, int ldj_init, int yb_width, hipStream_t stream);
// s: saved fp32 s, or (s_is_shat_bf16) the bf16 conditioner output s_hat (s recomputed)
void nf_launch_coupling_bwd(const void* s, int s_is_shat_bf16, long ld_s, const float* gy,
                            long ld_gy, const float* x, long ld_x, float c_scalar,
                            const float* c_row, void* dst, int dst_is_bf16, long ld_dst, float* gx,
                            long ld_gx, int B, int Dh, float scale, int gx_accumulate,
                            int dst_pad_to, hipStream_t stream);

// spline.hip: rational-quadratic spline coupling transform. params [B, (3K-1) Dh] plane-major
// (fp32 or bf16), x / y / g_out / gx [B, Dh] fp32 contiguous, ldj / g_ldj [B]; 2 <= K <= 32.
// x is the input of the direction taken (the inverse reads y there), in the backward too.
void nf_launch_rqs_fwd(const void* params, int params_is_bf16, const float* x, float* y,
                       float* ldj, int B, int Dh, int K, float bound, int inverse, int ldj_init,
                       hipStream_t stream);
// dparams in the dtype of params, every column written
void nf_launch_rqs_bwd(const void* params, int params_is_bf16, const float* x, const float* g_out,
                       const float* g_ldj, void* dparams, float* gx, int B, int Dh, int K,
                       float bound, int inverse, hipStream_t stream);

// dsf.hip: deep sigmoidal flow transformer. params [B, 3H D] plane-major (fp32 or bf16; planes
// ua, b, uw), x / y / g_out / gx [B, D] fp32 contiguous, ldj / g_ldj [B]; 1 <= H <= 32.
// The forward's x is the input of the direction taken (the inverse reads y there); the
// backward's x is the x-side value in both directions (the inverse's output).
void nf_launch_dsf_fwd(const void* params, int params_is_bf16, const float* x, float* y,
                       float* ldj, int B, int D, int H, int inverse, int ldj_init,
                       hipStream_t stream);
// dparams in the dtype of params, every column written
void nf_launch_dsf_bwd(const void* params, int params_is_bf16, const float* x, const float* g_out,
                       const float* g_ldj, void* dparams, float* gx, int B, int D, int H,
                       int inverse, hipStream_t stream);

// sylvester.hip: fused K-layer Sylvester flow stack, fp32, 1 <= D <= 64, 0 <= H <= 16, K >= 1.
// Every parameter (gradient) tensor is [rows, K, width] with a dense inner [K, width] block and a
// row stride in elements (0 = shared); widths: R1 / R2 D(D-1)/2 (strict upper, packed by
// column), d1 / d2 / b D, V H D. z / zK / gz / dz [N, D], ldj / gl [N], saved [N, K, D] dense;
// flips: K host bytes (layer k reverses the coordinates).
struct NfSylParams {
  const float *R1, *R2, *d1, *d2, *b, *V;
  long rs_R1, rs_R2, rs_d1, rs_d2, rs_b, rs_V;
};
struct NfSylGrads {
  float *R1, *R2, *d1, *d2, *b, *V;
  long rs_R1, rs_R2, rs_d1, rs_d2, rs_b, rs_V;
};
// saved may be null (no backward will follow)
void nf_launch_sylvester_fwd(const float* z, const NfSylParams& p, const unsigned char* flips,
                             float* zK, float* ldj, float* saved, int N, int D, int K, int H,
                             hipStream_t stream);
// per-row gradients, every entry written
void nf_launch_sylvester_bwd(const float* saved, const NfSylParams& p, const unsigned char* flips,
                             const float* gz, const float* gl, float* dz, const NfSylGrads& g,
                             int N, int D, int K, int H, hipStream_t stream);

// stein.hip: all-pairs SVGD direction and Stein-kernel row sums (KSD), fp32, 1 <= D <= 64.
// x / score [N, D] with row strides ldx / lds in elements and unit inner stride; the bandwidth is
// *h_dev when h_dev is not null, else h_host; kind 0 = rbf, 1 = imq. S = nf_stein_splits(N, D,
// j_splits) partial sums per output element go through work ([S, N, D] floats for svgd, [S, N]
// for ksd) and are added in fixed order; phi [N, D], rows / diag [N] dense, every entry written.
int nf_stein_splits(int N, int D, int j_splits);   // j_splits = 0: chosen from (N, D) alone
void nf_launch_stein_svgd(const float* x, long ldx, const float* score, long lds,
                          const float* h_dev, float h_host, int kind, int S, float* phi,
                          float* work, int N, int D, hipStream_t stream);
void nf_launch_stein_ksd(const float* x, long ldx, const float* score, long lds,
                         const float* h_dev, float h_host, int kind, int S, float* rows,
                         float* diag, float* work, int N, int D, hipStream_t stream);

// glm.hip: log-density and score of B parameter rows of a generalised linear model against N
// data rows, fp32, 1 <= D <= 64. theta [B, D] / X [N, D] with row strides ldt / ldx in elements
// and unit inner stride, y [N] dense; family 0 = bernoulli, 1 = poisson, 2 = gaussian (inv_var).
// The prior precision is prec_dev[D] when not null, else prec_host; has_prior = 0: flat prior.
// S = nf_glm_splits(B, N, D, n_splits) partial sums per output element go through work
// ([S, B, D + 1] floats) and are added in fixed order; logp [B], grad [B, D] dense, all written.
int nf_glm_splits(int B, int N, int D, int n_splits);   // n_splits = 0: chosen from (B, N, D)
void nf_launch_glm_logp_grad(const float* theta, long ldt, const float* X, long ldx,
                             const float* y, const float* prec_dev, float prec_host,
                             int has_prior, int family, float inv_var, float scale, int S,
                             float* logp, float* grad, float* work, int B, int N, int D,
                             hipStream_t stream);

// glm_hess.hip: the Newton statistics of the same posteriors in one pass: logp [B], grad [B, D]
// and hess [B, D, D] = scale sum_n w(eta_bn) x_n x_n^T + diag(prec), the negative Hessian of
// logp, exactly symmetric. Arguments as for glm.hip; S = nf_glm_hess_splits(B, N, D, n_splits)
// partial sums go through work ([S, B, D D + D + 1] floats) and are added in fixed order.
int nf_glm_hess_splits(int B, int N, int D, int n_splits);   // n_splits = 0: chosen from (B, N, D)
void nf_launch_glm_logp_grad_hess(const float* theta, long ldt, const float* X, long ldx,
                                  const float* y, const float* prec_dev, float prec_host,
                                  int has_prior, int family, float inv_var, float scale, int S,
                                  float* logp, float* grad, float* hess, float* work, int B, int N,
                                  int D, hipStream_t stream);

// glm_hmc.hip: one HMC trajectory (L leapfrog steps, 1 <= L <= 1024) and its accept step for B
// chains on a GLM posterior, fp32, 1 <= D <= 64; data, family and prior as for glm.hip. theta0
// [B, D] with row stride ldt, everything else dense: p0 / grad0 [B, D], logp0 / eps / log_u [B],
// minv [D] or null (identity mass). Written: theta_prop / p_prop (the trajectory's end),
// theta_out / logp_out / grad_out (the state after the accept step; bitwise the inputs on a
// reject), accept (0 or 1) and dH [B]. No output may alias an input. rows = chains per workgroup,
// one of nf_glm_hmc_rows' values; a chain's result does not depend on it.
int nf_glm_hmc_rows(int B, int D, int rows);   // rows = 0: chosen from (B, D); -1: not built
void nf_launch_glm_hmc_trajectory(const float* theta0, long ldt, const float* p0,
                                  const float* logp0, const float* grad0, const float* eps,
                                  const float* minv, const float* log_u, int L, const float* X,
                                  long ldx, const float* y, const float* prec_dev, float prec_host,
                                  int has_prior, int family, float inv_var, float scale, int rows,
                                  float* theta_prop, float* p_prop, float* theta_out,
                                  float* logp_out, float* grad_out, float* accept, float* dH,
                                  int B, int N, int D, hipStream_t stream);

// elbo.hip
void nf_launch_target_logp_grad(int kind, const float* A, long lda, const float* Bh, long ldb,
                                float* gA, long ldga, float* gB, long ldgb, int grad_accumulate,
                                const float* params, float p0, float p1, float p2, float cst,
                                const float* beta_ptr, float beta_host, float row_weight,
                                const float* logq0, const float* ldj, float* logp_out,
                                float* frow_out, int B, int Dh, hipStream_t stream);
void nf_launch_bernoulli_logits(const void* logits, int is_bf16, long ldl_, const float* x, long ldx,
                                void* dlogits, long ldd, const float* coef_ptr, float coef_host,
                                float* logpx, int B, int P, hipStream_t stream);
// energy2d.hip: the reference's 2-D targets (U1-U4, trial1): log p, gscale * beta * grad log p,
// optional ELBO row logq0 - ldj - beta log p; z [B][2] fp32 rows (ldz, ldg even)
void nf_launch_energy2d(int kind, const float* z, long ldz, float* logp, float* grad, long ldg,
                        float gscale, const float* logq0, const float* ldj, const float* beta,
                        float* frow, int B, hipStream_t stream);

// sampling.hip
void nf_launch_reparam_sample(const float* mu, const float* logvar, uint64_t seed,
                              const int64_t* offset_ptr, int64_t offset_host, uint32_t stream_id,
                              float* z, long ldz, float* eps, long lde, void* zbf, int zbf_is_bf16,
                              long ldzb, int nbf, float* logq0, int B, int D, hipStream_t stream);
void nf_launch_normal_fill(float* out, long n, uint64_t seed, const int64_t* offset_ptr,
                           int64_t offset_host, uint32_t stream_id, hipStream_t stream);
void nf_launch_reparam_grad(const float* g_lo, long ldlo, const float* g_hi, long ldhi,
                            const float* eps, long lde, const float* logvar, float* partial,
                            int npartial, float* gmu, float* glv, int B, int D, int Dl,
                            hipStream_t stream);

// optim.hip
void nf_launch_flat_optimizer(int kind, float* p, const float* g, float* m, float* v, void* pbf,
                              long n, float lr, float b1, float b2, float eps, float wd,
                              const float* step_ptr, float step_host, const float* gscale_ptr,
                              float gscale_host, const float* skip_ptr, float warmup,
                              hipStream_t stream);
// diagnostics: hold `blocks` CU slots for `usec` us (collective-occupancy emulation)
void nf_launch_cu_hold(int blocks, float usec, hipStream_t stream);
void nf_launch_sumsq_guard(const float* x, long n, float* partial, int npartial, float* out_sumsq,
                           float* out_skip, float* out_scale, float max_norm, float base_scale,
                           hipStream_t stream);

// gemm.hip (bf16 MFMA, fp32 accumulate)
// mask_out: optional ReLU bitmask [M][N/8] bytes (bit e of byte n/8 <-> column n+e) written by
// the forward epilogue; aux_is_bits: the dgrad's ReLU mask `aux` is such a bitmask (ld in bytes)
// Lane-private mask (mask_lanes = 1 / aux_is_bits = 2): the same M*N/8 bytes in the 256x256
// kernel's accumulator order (gemm_tile.h, "Lane-private ReLU mask"), written and read only by
// that kernel on whole 256x256 tiles. These launchers return NF_LANES_OK (0) when they launched,
// and launch nothing otherwise: NF_LANES_SHAPE when the layout is not defined for the shape or
// alignment (both ends of a product pair then agree, and the caller uses the row-major mode),
// NF_LANES_KERNEL when the shape fits but the call routes to the 128x128 kernel.
enum { NF_LANES_OK = 0, NF_LANES_SHAPE = 1, NF_LANES_KERNEL = 2 };
int nf_launch_gemm_nt(const void* x, long ldx, const void* W, long ldw, const void* bias, void* y,
                      long ldy, int M, int N, int K, int relu, hipStream_t stream,
                      void* mask_out = nullptr, long ld_mask = 0, int mask_lanes = 0);
// what the pair (forward over K_fwd writing the mask, input gradient over K_bwd reading it)
// would return for lane mode right now, without launching anything
int nf_gemm_mask_lanes_route(int M, int N, int K_fwd, int K_bwd, int bwd_wt);
int nf_launch_gemm_nn(const void* dy, long lddy, const void* W, long ldw, const void* aux,
                      long ld_aux, void* dx, long lddx, int dx_is_f32, int accumulate, int M,
                      int N, int K, hipStream_t stream, int aux_is_bits = 0);
// y[M][N] = x W^T with bf16 operands and an fp32 output (no rounding of the accumulator)
void nf_launch_gemm_nt_f32out(const void* x, long ldx, const void* W, long ldw, float* y, long ldy,
                              int M, int N, int K, hipStream_t stream);
// gemm_fp.hip: exact fp32 / fp64 GEMM on the f32 / f64 MFMA, C (+)= Aop Bop^T (+ bias),
// dbias = row sums of Aop (see the kernel header for the operand layouts)
// split-K: `work` holds splits * (M * N + M) elements of the output dtype (nf_gemm_fp_splits
// picks the count: 1 = no split, work unused)
int nf_gemm_fp_splits(int M, int N, int K);
void nf_launch_gemm_fp(int is_f64, const void* A, long lda, int a_kmajor, const void* B, long ldb,
                       int b_kmajor, const void* bias, void* C, long ldc, void* dbias, int M, int N,
                       int K, int accumulate, hipStream_t stream, void* work = nullptr,
                       int splits = 1);
void nf_launch_gemm_tn(const void* dy, long lddy, const void* x, long ldx, float* dW, long lddw,
                       float* db, int M, int N, int K, int splits, float* work,
                       hipStream_t stream);
long nf_gemm_tn_workspace(int M, int N, int splits);
// grouped weight gradients dW_p = dy_p^T x_p, db_p = colsum(dy_p) (p < 4), one GEMM launch +
// one reduce launch
struct NfTnProblem {
  const void* dy; long lddy;
  const void* x; long ldx;
  float* dW; long lddw;
  float* db;
  int M, N, K;
  const unsigned char* skip = nullptr;   // masked (MADE) weights: all-zero 128x128 tiles of dW
  const unsigned char* cmask = nullptr;  // [M][N] 0/1: zero the masked entries of dW
  // gemm256_tn_multi only: the 256x256 tiles to compute (all-masked tiles are left out of the
  // numbering and never written), ntiles_active of them; -1 = every tile
  const unsigned short* tiles = nullptr;
  int ntiles_active = -1;
  // gemm256_tn_multi e4m3 launches: dy / x dequantisation scales = f8_scales[sa_idx / sb_idx]
  int sa_idx = -1, sb_idx = -1;
};
long nf_gemm_tn_group_workspace(int nprob, const NfTnProblem* pr);
void nf_launch_gemm_tn_group(int nprob, const NfTnProblem* pr, float* work, hipStream_t stream);
// gemm256.hip: 256x256 8-phase kernel (forward / input-gradient products)
// krange: optional per-256-column-tile K ranges [lo, hi) of a MADE-masked weight
int nf_launch_gemm256_nt(const void* x, long ldx, const void* W, long ldw, const void* bias,
                         void* y, long ldy, int M, int N, int K, int relu, hipStream_t stream,
                         void* mask_out = nullptr, long ld_mask = 0,
                         const int* krange = nullptr, int mask_lanes = 0);
int nf_launch_gemm256_nn(const void* dy, long lddy, const void* W, long ldw, const void* aux,
                         long ld_aux, void* dx, long lddx, int dx_is_f32, int accumulate, int M,
                         int N, int K, hipStream_t stream, int aux_is_bits = 0,
                         const int* krange = nullptr, int krange_segs = 1, int w_kmajor = 0);
void nf_gemm256_set_persist(int on);
int nf_gemm256_get_persist();
int nf_gemm256_set_reserve(int cus);   // cus < 0: query; returns the previous value
int nf_gemm256_set_pair(int mode);     // MADE tile pairing 0 off / 1 auto / 2 always; < 0: query
// input gradient with W given transposed (Wt [N][K]): NT instantiation, bf16 (ReLU-mask) epilogue
int nf_launch_gemm256_nt_dgrad(const void* dy, long lddy, const void* Wt, long ldwt,
                               const void* aux, long ld_aux, int aux_is_bits, void* dx,
                               long lddx, int M, int N, int K, hipStream_t stream);
// layout.hip: batched bf16 transposes (TrDesc table on the device)
void nf_launch_transpose_bf16_batched(const void* desc, int n, int total_tiles,
                                      hipStream_t stream);
// last conditioner product of coupling layer l with its coupling forward fused (EPI_CPL_FWD)
void nf_launch_gemm256_nt_cpl(const void* h, long ldh, const void* W, long ldw, int w_rows,
                              const void* bias, void* st, long ld_st, int M, int K, int Dh,
                              const float* x, long ld_x, float* y, long ld_y, void* yb, long ld_yb,
                              int yb_width, float* ldjp, long ld_ldjp, int ldj_init, float scale,
                              hipStream_t stream, int inverse = 0);
// input gradient of coupling layer l's conditioner (fp32, + G) fused with coupling layer l-1's
// backward: writes dst (bf16 [dS_hat | dT | 0]) and gx; G itself is not written
// e4m3 operand scales of an fp8 product: sa (A, per-tensor), sb (B, per-row) and the optional
// e4m3 copy q of the output under a delayed per-tensor scale (ops/fp8.py DelayedScale)
struct NfF8Operands {
  const float* sa;
  const float* sb;
  void* q;
  long ldq;
  const float* q_amax_prev;
  float* q_scale_out;
  float* q_amax_cur;
};
void nf_launch_gemm256_nn_cpl(const void* dy, long lddy, const void* W, long ldw, const float* G,
                              long ldg, int M, int N, int K, const void* s_hat, long ld_s,
                              const float* x, long ld_x, void* dst, long ld_dst, int dst_pad,
                              float* gx, long ld_gx, int Dh, float scale, float c,
                              hipStream_t stream, int w_kmajor = 0, const int* krange = nullptr,
                              int krange_segs = 1, int mode = 0, const NfF8Operands* f8 = nullptr,
                              int x_bf16 = 0, int g_in_bf16 = 0, int gx_bf16 = 0);
void nf_launch_gemm256_fp8_dgrad(const void* dyq, long lddy, const float* sa, const void* wtq,
                                 long ldwt, const float* sb, const void* aux, long ld_aux,
                                 int aux_bits, void* dx, long lddx, int M, int N, int K,
                                 const int* krange, int krange_segs, void* dxq, long lddxq,
                                 const float* q_amax_prev, float* q_scale_out, float* q_amax_cur,
                                 hipStream_t stream);
void nf_launch_gemm256_maf_fwd(const void* h, long ldh, int f8, const float* hs, const void* W,
                               long ldw, const float* ws, const void* bias, const int* krange,
                               void* s_out, long ld_s, int M, int K, int D, const float* x,
                               long ld_x, float* u, long ld_u, void* ubf, long ld_ub, float* ldjp,
                               long ld_ldjp, int ldj_init, float bound, void* uq, long lduq,
                               const float* q_amax_prev, float* q_scale_out, float* q_amax_cur,
                               hipStream_t stream, int x_bf16 = 0);
int nf_launch_gemm256_tn_partials(const void* dy, long lddy, const void* x, long ldx, float* C,
                                  long ldc, long slab_stride, float* dbias, int M, int N, int K,
                                  int splits, hipStream_t stream);
// many dense weight gradients (no split-K, one 256x256 tile per block): tiles numbered problem
// after problem, one launch computes [tile0, tile0 + ntiles)
int nf_gemm256_tiles(int M, int N);
void nf_launch_gemm256_tn_multi(int nprob, const NfTnProblem* pr, int tile0, int ntiles,
                                hipStream_t stream, const float* f8_scales = nullptr,
                                int layout = 0);
// layout: 0 = dy [K][M], x [K][N] (batch-major, TN); 1 = x given transposed [N][K] (k-major);
// 2 = dy given transposed [M][K] - the operand-layout A/B (bench/wgrad_bench.py --probe)
// mode: 0 auto, 1 force 128x128, 2 force 256x256; depth: half-tiles in flight (3 or 4)
int nf_gemm_set_mode(int mode);
// fp8.hip (OCP e4m3): per-row quantisation and the MX-scaled K=128 MFMA GEMM
void nf_launch_fp8_quant_rows(const void* x, int x_is_bf16, long ldx, int R, int C, void* q,
                              long ldq, int Cq, float* scale, hipStream_t stream);
// fp8.hip: deterministic column sums s * sum_k q[k][n] of up to 40 e4m3 [K][N] tensors (the
// bias gradients of the e4m3 weight-gradient launches); part = nf_fp8_colsum_workspace floats
long nf_fp8_colsum_workspace(int n, const int* N);
void nf_launch_fp8_colsum(int n, const void* const* q, const long* ld, const int* K, const int* N,
                          float* const* out, const int* sidx, const float* scales, float* part,
                          hipStream_t stream);
void nf_launch_fp8_quant_tensor(const void* x, int x_is_bf16, long ldx, int R, int C, void* q,
                                long ldq, int Cq, const float* amax_prev, float* scale_out,
                                float* amax_cur, hipStream_t stream);
void nf_launch_gemm_fp8_nt(const void* xq, long ldx, const float* sx, int sx_per_row,
                           const void* wq, long ldw, const float* sw, const void* bias, void* y,
                           long ldy, int M, int N, int K, int relu, const int* krange,
                           void* yq, long ldyq, const float* q_amax_prev, float* q_scale_out,
                           float* q_amax_cur, hipStream_t stream);
int nf_gemm_tn_splits(int M, int N, int K);
// the 256x256 kernels' auto rule (a tile per CU, K >= 256; gemm_set_mode)
bool nf_gemm_prefer_256(int M, int N, int K);
// gemm256.hip F8 instantiation: same contract as nf_launch_gemm_fp8_nt on 256x256 tiles
// (krange per 256-column tile)
void nf_launch_gemm256_fp8_nt(const void* xq, long ldx, const float* sx, int sx_per_row,
                              const void* wq, long ldw, const float* sw, const void* bias, void* y,
                              long ldy, int M, int N, int K, int relu, const int* krange,
                              void* yq, long ldyq, const float* q_amax_prev, float* q_scale_out,
                              float* q_amax_cur, hipStream_t stream,
                              unsigned char* mask_out = nullptr, long ld_mask = 0);

// planar.hip / radial.hip (fused K-layer stacks; per-row parameter gradients)
void nf_launch_planar_fwd(const float* z, const float* W, const float* U, const float* B, float* zK,
                          float* ldj, float* saved, int N, int D, int K, int per_sample,
                          int broadcast, hipStream_t stream);
void nf_launch_planar_bwd(const float* saved, const float* W, const float* U, const float* B,
                          const float* gz, const float* gl, float* dz, float* dW, float* dU,
                          float* dB, int N, int D, int K, int per_sample, int broadcast,
                          hipStream_t stream);
// shared parameters, D <= 16, K * per(D) <= 256: recompute-from-z0 backward with in-kernel
// parameter-gradient reduction (part: nblk * K * (2 per + 1) floats)
int nf_planar_shared_per(int D);
int nf_planar_shared_blocks(int N);
void nf_launch_planar_bwd_shared(const float* z0, const float* W, const float* U, const float* B,
                                 const float* gz, const float* gl, float* dz, float* dW, float* dU,
                                 float* dB, float* part, int nblk, int N, int D, int K,
                                 int broadcast, hipStream_t stream);
void nf_launch_radial_fwd(const float* z, const float* Z0, const float* AL, const float* BE,
                          float* zK, float* ldj, float* saved, int N, int D, int K,
                          int per_sample, hipStream_t stream);
void nf_launch_radial_bwd(const float* saved, const float* Z0, const float* AL, const float* BE,
                          const float* gz, const float* gl, float* dz, float* dZ0, float* dA,
                          float* dBe, int N, int D, int K, int per_sample, hipStream_t stream);
// inverses of the paper-variant planar stack and of the radial stack: x from y, layers undone
// K-1 .. 0, saved[k] = the preimage under layer k; the backwards write per-row gradients
void nf_launch_planar_inv(const float* y, const float* W, const float* U, const float* B, float* x,
                          float* ldj, float* saved, int N, int D, int K, int per_sample,
                          hipStream_t stream);
void nf_launch_planar_inv_bwd(const float* saved, const float* W, const float* U, const float* B,
                              const float* gx, const float* gl, float* dy, float* dW, float* dU,
                              float* dB, int N, int D, int K, int per_sample, hipStream_t stream);
void nf_launch_radial_inv(const float* y, const float* Z0, const float* AL, const float* BE,
                          float* x, float* ldj, float* saved, int N, int D, int K,
                          int per_sample, hipStream_t stream);
void nf_launch_radial_inv_bwd(const float* saved, const float* Z0, const float* AL,
                              const float* BE, const float* gx, const float* gl, float* dy,
                              float* dZ0, float* dA, float* dBe, int N, int D, int K,
                              int per_sample, hipStream_t stream);

// masked (MADE) GEMMs: per-N-tile K ranges [ntn][2] / per-tile skip flags [ntm*ntn] (128x128 tiles)
void nf_launch_gemm_nt_masked(const void* x, long ldx, const void* W, long ldw, const void* bias,
                              void* y, long ldy, int M, int N, int K, int relu, const int* krange,
                              hipStream_t stream, const int* krange256 = nullptr);
void nf_launch_gemm_nn_masked(const void* dy, long lddy, const void* W, long ldw, const void* aux,
                              long ld_aux, void* dx, long lddx, int dx_is_f32, int accumulate, int M,
                              int N, int K, const int* krange, hipStream_t stream,
                              const int* krange256 = nullptr, int krange256_segs = 1,
                              const void* Wt = nullptr, long ldwt = 0);
void nf_launch_gemm_tn_masked(const void* dy, long lddy, const void* x, long ldx, float* dW,
                              long lddw, float* db, int M, int N, int K, int splits, float* work,
                              const unsigned char* skip, hipStream_t stream);

// maf.hip: masked autoregressive flow transform (density direction) fwd / bwd
void nf_launch_maf_fwd(const float* x, long ldx, const void* o, long ldo, int B, int D, float bound,
                       float* u, long ldu, void* ubf, long ldub, void* uq, long lduq,
                       const float* amax_prev, float* scale_out, float* amax_cur, float* ldj,
                       int ldj_init, hipStream_t stream);
void nf_launch_maf_bwd(const float* gu, long ldg, const float* u, long ldu, const void* s_raw,
                       long lds, int B, int D, float bound, float c_ldj, void* dout, long lddo,
                       float* gx, long ldgx, hipStream_t stream, const float* c_row = nullptr);
// maf.hip: gated IAF update (o = [m | s] bf16 from the MADE GEMM)
void nf_launch_iaf_gate_fwd(const void* o, long ldo, const float* z, long ldz, int B, int D,
                            float gate_bias, float* y, long ldy, float* ldj, hipStream_t stream,
                            void* ybf = nullptr, long ldyb = 0);
void nf_launch_iaf_gate_bwd(const float* gy, long ldg, const float* gl, const float* z, long ldz,
                            const void* o, long ldo, int B, int D, float gate_bias, void* dout,
                            long lddo, float* gz, long ldgz, hipStream_t stream);
// fp8.hip: layer-strided per-row weight quantisation (rows r -> layer r / rows_per)
void nf_launch_fp8_quant_rows_strided(const void* x, int x_is_bf16, long ldx, long layer_stride,
                                      int rows_per, int R, int C, void* q, long ldq, int Cq,
                                      float* scale, hipStream_t stream);

// vae.hip: whole training step of the amortized planar-flow VAE (reference main workload):
// phase 1 row-parallel forward + input-gradient chain, phase 2 batch-reduction weight gradients
struct NfVaeParams {
  const float* enc_W[4];
  const float* enc_b[4];
  const float* enc_Wo;
  const float* enc_bo;
  const float* dec_W[4];
  const float* dec_b[4];
  const float* dec_Wo;
  const float* dec_bo;
};
struct NfVaeGrads {
  float* enc_W[4];
  float* enc_b[4];
  float* enc_Wo;
  float* enc_bo;
  float* dec_W[4];
  float* dec_b[4];
  float* dec_Wo;
  float* dec_bo;
};
size_t nf_vae_rows_lds_bytes(int Din, int dz, int K, int De);
void nf_launch_vae_step(const NfVaeParams& prm, const float* x, const float* eps_in, unsigned seed,
                        const long* offset, const float* beta, int B, int Din, int dz, int K,
                        int L, float* ws_eact, float* ws_egrad, float* ws_gphi, float* ws_zk,
                        float* ws_dact, float* ws_dgrad, float* ws_dl, float* frow, float* loss,
                        float* zk_out, float* ldj_out, const NfVaeGrads& grd, hipStream_t stream);

// made_sweep.hip: the sequential direction of a MADE-conditioned flow (MAF sampling, IAF
// inverse) as one degree sweep. W[l] [H, D or H] / b[l] [H] are the L hidden layers, Wo [2D, H] /
// bo [2D] the output layer (rows i = m, i + D = s), all fp32, unmasked, unit inner stride with row
// strides in elements; perm [D] and ubeg [L, D + 2] (ubeg[l][t] = number of layer-l units of
// degree < t) are int32 device arrays; kind 0 = maf_sample (param = bound), 1 = iaf_gated (param =
// gate_bias), 2 = iaf_affine (param = scale). x [B, D] and ldj [B] are written for every row.
#define NF_MADE_SWEEP_MAX_HIDDEN 4
struct NfMadeSweep {
  const float* W[NF_MADE_SWEEP_MAX_HIDDEN];
  const float* b[NF_MADE_SWEEP_MAX_HIDDEN];
  long ldw[NF_MADE_SWEEP_MAX_HIDDEN];
  const float* Wo;
  long ldo;
  const float* bo;
  const float* v;
  long ldv;
  const float* ctx;   // [B, H] added to layer 1's pre-activation, or null
  long ldc;
  const int* perm;
  const int* ubeg;
  float* x;
  long ldx;
  float* ldj;
  int B, D, H, L, kind;
  float param;
};
// rows per block the launcher picks for (D, H, L): the largest tile whose LDS state fits the
// budget it requests; 0 = the shape is not supported
int nf_made_sweep_rows(int D, int H, int L);
void nf_launch_made_sweep(const NfMadeSweep& s, hipStream_t stream);

// dsf_sweep.hip: the inverse of a MADE-conditioned deep sigmoidal flow layer (y -> z) as one
// degree sweep. The tensors are those of NfMadeSweep (v = y, x = z; kind and param unused) except
// the output layer: Wo [3U D, H] / bo [3U D] plane-major (row k D + i is plane k of coordinate i;
// planes [0, U) raw slopes, [U, 2U) shifts, [2U, 3U) mixture logits), 1 <= U <= 32. ldj [B] is
// minus sum_i log dy_i/dz_i at the recovered z.
// rows per block for (D, H, L, U); 0 = the shape is not supported
int nf_dsf_sweep_rows(int D, int H, int L, int U);
void nf_launch_dsf_sweep(const NfMadeSweep& s, int U, hipStream_t stream);

// rqs_sweep.hip: the sequential direction of a MADE-conditioned rational-quadratic spline layer
// (y -> z with T(z) = y) as one degree sweep. The tensors are those of NfMadeSweep (v = y, x = z;
// kind and param unused) except the output layer: Wo [(3K - 1) D, H] / bo [(3K - 1) D] plane-major
// (row k D + i is plane k of coordinate i; planes [0, K) unnormalised widths, [K, 2K) heights,
// [2K, 3K - 1) interior derivatives), 2 <= K <= 32 bins on (-bound, bound), bound > 0. ldj [B] is
// minus sum_i log dy_i/dz_i at the recovered z.
// rows per block for (D, H, L, K); 0 = the shape is not supported
int nf_rqs_sweep_rows(int D, int H, int L, int K);
void nf_launch_rqs_sweep(const NfMadeSweep& s, int K, float bound, hipStream_t stream);

// sweep_adjoint.hip: the transpose of the degree sweeps' forward substitution, walking the degrees
// downwards: given gx = xbar - lbar e [B, D], d = dtau/dx [B, D] and, per coordinate, q = dtau/dp
// and c = lbar dlog d/dp [B, D, P] (coordinate-major: the P values of one coordinate are
// contiguous), it solves for w [B, D] (the cotangent of v), pbar = q w + c [B, D, P] (may alias c)
// and a[l] = hbar_l [h_l > 0] [B, H] (the cotangents of the hidden pre-activations). h[l] [B, H]
// are the hidden activations at the solution (used only for > 0); W[l] / Wo are the unmasked fp32
// weights of NfMadeSweep with Wo [P D, H] plane-major, 1 <= P <= NF_SWEEP_ADJOINT_MAX_P.
#define NF_SWEEP_ADJOINT_MAX_P 96
struct NfSweepAdjoint {
  const float* W[NF_MADE_SWEEP_MAX_HIDDEN];
  long ldw[NF_MADE_SWEEP_MAX_HIDDEN];
  const float* h[NF_MADE_SWEEP_MAX_HIDDEN];
  long ldh[NF_MADE_SWEEP_MAX_HIDDEN];
  float* a[NF_MADE_SWEEP_MAX_HIDDEN];
  long lda[NF_MADE_SWEEP_MAX_HIDDEN];
  const float* Wo;
  long ldo;
  const int* perm;
  const int* ubeg;
  const float* gx;
  long ldg;
  const float* d;
  long ldd;
  const float* q;     // [B, D, P] contiguous
  const float* c;     // [B, D, P] contiguous
  float* pbar;        // [B, D, P] contiguous
  float* w;
  long ldwo;
  int B, D, H, L, P;
};
// rows per block for (D, H, L, P); 0 = the shape is not supported
int nf_sweep_adjoint_rows(int D, int H, int L, int P);
void nf_launch_sweep_adjoint(const NfSweepAdjoint& s, hipStream_t stream);

// lu_solve.hip: x = (P L U)^-1 (y - b) per batch row and its transpose, against a packed factor
// A [D, D] (mode 0 = LU: strict lower triangle L with an implied unit diagonal, upper triangle U
// with its diagonal; mode 1 = LOWER: the lower triangle with its diagonal is the one factor, the
// strict upper triangle is never read), W = (L U)[perm, :].
//   transpose 0: s[:, perm[i]] = y[:, i] - bias[i]; L z = s; U x = z; x stored.
//   transpose 1: U^T q = y; L^T g = q; g[:, perm] stored (W^-T y; bias unused).
// M is the EQUATION-major orientation of the factor, M[k][i] = the coefficient of unknown k in
// equation i: A^T for transpose 0, A itself for transpose 1. fp32, unit inner strides with row
// strides in elements; perm (int32 device array, clamped to [0, D)) and bias may be null.
struct NfLuSolve {
  const float* M;
  long ldm;
  const float* y;
  long ldy;
  const int* perm;
  const float* bias;
  float* x;
  long ldx;
  int B, D, mode, transpose;
};
// rows per block the launcher picks for D: the largest tile whose LDS state fits the budget it
// requests; 0 = D is not supported (1 <= D <= 2048 is)
int nf_lu_solve_rows(int D);
void nf_launch_lu_solve(const NfLuSolve& s, hipStream_t stream);
