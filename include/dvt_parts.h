/* Component entry points for tests; no reference counterpart.
 *
 * The exact-fp32 kernels that the stage-2 and stage-3 training steps (and the fp32 extractor's 128 x 128 tile) are built
 * from, one call per kernel, so that tests/test_gpu_parts.py can hold each of them to fp64 element by element at shapes
 * the trainers never give them (partial tiles, uneven k-splits, padded query blocks, idle lanes of a 384-wide row).
 *
 * Every function is a thin forwarder in the translation unit that owns the kernel: it adds no kernel and changes no
 * launch.  It validates pointers and shapes and returns DVT_E_BADARG (-1) before any launch, takes a hipStream_t as
 * `void* stream` and does not synchronise.  All pointers are device pointers, 16-byte aligned, fp32 unless said otherwise.
 *
 * The block code that the stage-2 and the stage-3 step share is compiled once, in csrc/dvt_block_train.hip: its
 * dvt_parts_* functions reach the one copy of those kernels and launchers, so tests/test_gpu_parts.py holds exactly what
 * both trainers launch.
 *
 * Developer instrumentation in the class of dvt_tune_set: not API, ABI version unchanged.
 */
#ifndef DVT_PARTS_H
#define DVT_PARTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dvt_gemm_f32_glds.hip (dvt_parts_gemm_ex), dvt_gemm_f32_big.hip (dvt_parts_linear_big_epi) ----------------- */
/* Mirror of the internal DvtGemmEx (csrc/dvt_common.h), field for field:
 *   layout 0: C[M][N] = A[M][K] . B[N][K]^T (+ bias[n]);  1: C = A[M][K] . B[K][N] (N % 64 == 0);
 *   layout 2: C = A[K][M]^T . B[K][N] (M % 64 == N % 64 == 0; colsum[m] += sum_k A[k][m]).
 * K % 64 == 0, lda % 4 == ldb % 4 == 0.  accumulate: fp32 atomic adds into C, the reduction split over workgroups (unbatched
 * only).  nb0 * nb1 > 1: batched over (b0, b1) with element strides s?0 / s?1.  smul / rowsub / oscale: C = oscale * smul (.)
 * (A B^T - rowsub), batched layout 0 with K == 64 only; smul is indexed like C, rowsub[(b0 * nb1 + b1) * M + m]. */
typedef struct DvtPartsGemmEx {
  int32_t layout;
  int32_t pad0_;
  const float* A;
  const float* B;
  float* C;
  int32_t M, N, K, lda, ldb, ldc;
  const float* bias;
  float* colsum;
  int32_t accumulate;
  int32_t nb0, nb1;
  int32_t pad1_;
  int64_t sA0, sA1, sB0, sB1, sC0, sC1;
  const float* smul;
  const float* rowsub;
  float oscale;
  int32_t pad2_;
} DvtPartsGemmEx;
int dvt_parts_gemm_ex(const DvtPartsGemmEx* g, void* stream);

/* y[m][n] = epi(x[m][k] . w[n][k]^T + b).  epi 0: dvt_linear_fwd_big (the 128 x 128 x 32 tile where m % 128 == n % 128 ==
 * k % 32 == 0, else the 64 x 64 LDS-DMA kernel where k % 64 == 0, else the register-staged kernel; n % 4 == k % 4 == 0).
 * epi 1: exact-erf GELU, epi 2: y += gamma[n] * (.) -- both on the 128 x 128 tile only (other shapes: DVT_E_BADARG). */
int dvt_parts_linear_big_epi(const float* x, const float* w, const float* b, float* y, int m, int n, int k, int epi,
                             const float* gamma, void* stream);

/* ---- dvt_block_train.hip (lin_fwd .. loss_rows, add_ln, shared by stages 2 and 3) and dvt_stage2.hip (softmax, pos_grad) -- */
/* lin_fwd / lin_bwd exactly as the trainers call them; both obey dvt_tune_set(18, mask), the side-stream fork of the
 * weight gradient included (joined before the call returns to the caller's stream order).
 *   y[R][n] = x[R][k] . w[n][k]^T + b
 *   dx[R][k] = dy[R][n] . w[n][k] (dx may be NULL);  dw[n][k] += dy^T . x;  db[n] += colsum(dy);  wT: scratch [k][n] or NULL
 * Shapes a selected kernel cannot take (k % 64 in the forward; n % 64, k % 64, R % 32, and R % 64 unless the 128 x 128
 * weight-gradient tile is selected and takes the shape) are DVT_E_BADARG. */
int dvt_parts_lin_fwd(const float* x, const float* w, const float* b, float* y, int R, int n, int k, void* stream);
int dvt_parts_lin_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* db, float* wT, int R,
                      int n, int k, void* stream);

/* s2_attn_rows_kernel.  mode 0: out[b][h][Tp][Tp] = softmax(scale * q k^T) over keys < T, rows and columns >= T zero;
 * rowop = q, keyop = k, both [batch * Tp][ld] with the head at columns 64 h.  mode 1: out = scale * P (.) (rowop keyop^T -
 * D[b][h][Tp]), rowop = d ao, keyop = v.  Tp % 128 == 0, 1 <= T <= Tp, ld_key % 4 == 0. */
int dvt_parts_attn_rows(int mode, const float* rowop, int ld_row, const float* keyop, int ld_key, const float* P,
                        const float* D, float* out, int batch, int heads, int T, int Tp, float scale, void* stream);
/* D[(b * C / 64 + h) * Tp + t] = sum_d dO[b * Tp + t][64 h + d] * O[..][64 h + d];  C % 64 == 0, R % Tp == 0 */
int dvt_parts_rowdot(const float* dO, const float* O, float* D, int R, int Tp, int C, void* stream);
/* LayerNorm backward, C in {384, 768, 1024}: dx = dres + rstd (g - mean(g) - xhat mean(g xhat)), dgamma += sum dy xhat,
 * dbeta += sum dy; dres may be NULL */
int dvt_parts_ln_bwd(int C, const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                     const float* dres, float* dx, float* dgamma, float* dbeta, int R, void* stream);
/* sum = a (+ b), xn = LayerNorm(sum) gamma + beta, per-row mean / rstd; rows t >= T of every image all zero.  a packed
 * [R / Tp][T][C] (a_packed) or padded [R][C]; b NULL, pos [T][C] (b_is_pos) or padded; sum_out may be NULL */
int dvt_parts_add_ln(int C, const float* a, int a_packed, const float* b, int b_is_pos, float* sum_out, const float* gamma,
                     const float* beta, float* xn, float* mean, float* rstd, int T, int Tp, int R, float eps, void* stream);
/* backward 0: a = gelu(h) (exact erf);  1: a *= gelu'(h) in place.  n4 float4 elements */
int dvt_parts_gelu(const float* h, float* a, int64_t n4, int backward, void* stream);
/* backward 0: S [rows][Tp] -> softmax(scale S) over keys < T in place, query rows (row % Tp) >= T and keys >= T zero (P unused);
 * backward 1: S = scale P (.) (S - rowsum(P (.) S)) in place.  Tp % 4 == 0 */
int dvt_parts_softmax(const float* P, float* S, int T, int Tp, int64_t rows, float scale, int backward, void* stream);
/* loss_rows<add>: dout [R][C], loss_out[4] = {l2 + 1 - cos, l2, 1 - cos, 0}, out (may be NULL) packed; acc: 64 floats of scratch, 8-byte
 * aligned (the two sums are added as 128-bit integers, in any order to the same bits).
 * target / out packed [R / Tp][T - n_prefix][C]; b is read with add only */
int dvt_parts_loss_rows(int C, const float* a, const float* b, const float* target, float* out, float* dout, float* acc,
                        int n_prefix, int T, int Tp, int R, int norm_batch, float* loss_out, int add, void* stream);
/* dpos[t][c] += sum_b dx[b * Tp + t][c], t < T;  C % 4 == 0 */
int dvt_parts_pos_grad(const float* dx, float* dpos, int batch, int T, int Tp, int C, void* stream);

/* ---- dvt_block_train.hip (ls_add_ln, ls_bwd) and dvt_stage3.hip (the embedding; s3_embed and s3_im2col launch the fp32
 * extractor's kernels of dvt_vit_f32.hip, which stage 3 runs) ---- */
/* sum = a + ls (.) f (ls NULL: sum = a), then as dvt_parts_add_ln (all rows padded [R][C]) */
int dvt_parts_ls_add_ln(int C, const float* a, const float* f, const float* ls, float* sum_out, const float* gamma,
                        const float* beta, float* xn, float* mean, float* rstd, int T, int Tp, int R, float eps, void* stream);
/* df = ls (.) dy, dls += sum_rows f (.) dy */
int dvt_parts_ls_bwd(int C, const float* dy, const float* f, const float* ls, float* df, float* dls, int R, void* stream);
/* token assembly x [batch * s_pad][dim] from the patch embedding y (same rows), prefix [n_prefix][dim] and pos
 * [pos_has_cls + n_tokens - n_prefix][dim]; and its backward (dprefix, dpos +=; the prefix rows of dx zeroed) */
int dvt_parts_s3_embed(const float* y, float* x, const float* prefix, const float* pos, int batch, int dim, int n_prefix,
                       int n_tokens, int s_pad, int pos_has_cls, void* stream);
int dvt_parts_s3_embed_bwd(float* dx, float* dprefix, float* dpos, int batch, int dim, int n_prefix, int n_tokens, int s_pad,
                           int pos_has_cls, void* stream);
/* col [batch * s_pad][k_patch] from img [batch][3][img_h][img_w]; prefix rows, padded rows and columns >= 3 patch^2 zero */
int dvt_parts_s3_im2col(const float* img, float* col, int batch, int patch, int stride, int img_h, int img_w, int grid_h,
                        int grid_w, int n_prefix, int s_pad, int k_patch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DVT_PARTS_H */
