/*
 * dvt_stage3.h -- C ABI of the stage-3 distillation step in libdvt_hip.so (gfx950).
 *
 * Replaces, for the reference's stage 3 (main_distillation.py, run by sample_scripts/stage3.sh), one training step of the
 * student `PretrainedViTWrapper` -- a whole DINOv2 ViT, every parameter trained, fp32 (the reference never autocasts):
 *   feats = norm(blocks(patch_embed(img) | prefix tokens + pos_embed))[:, n_prefix:]     (get_intermediate_layers, n=1, norm)
 *   loss  = F.mse_loss(feats, target) + 1 - F.cosine_similarity(feats, target, dim=-1).mean()
 *   loss.backward()
 * The optimizer step is dvt_adamw_step (include/dvt_stage2.h) over the same flat arenas.
 *
 * Configuration: DvtVitConfig (include/dvt_vit.h) as dvt_vit_config / dvt_vit_config_reg write it; s_pad must be a multiple
 * of 128 (the attention row kernels walk whole blocks of 128 queries), dim 384 / 768 / 1024, heads = dim / 64.
 *
 * Arithmetic: exact fp32 throughout, on the block code shared with the stage-2 step (csrc/dvt_block_train.hip): linear layers on the
 * 128 x 128 x 32 exact-fp32 MFMA tile, the softmax fused into the two [s_pad][s_pad] attention products, probabilities kept
 * for the backward pass, two-pass LayerNorm statistics, erf GELU.  Every block keeps its activations: about 0.18 GB per image
 * and block for ViT-B/14 at 518 x 518 (host code splits a batch that does not fit into slices, dvt_s3_train_slice).
 *
 * Opt-in mixed precision (dvt_s3_train_slice_pos_mp, gemm_mode 1): of the three GEMMs of each of a block's four linear layers
 * (qkv, proj, fc1, fc2), the forward y = x W^T + b and the data gradient dx = dy W run on the extractor's bf16 MFMA GEMM
 * (csrc/dvt_vit_gemm.hip, fp32 accumulation, fp32 output) with BOTH operands rounded to bf16, round to nearest even: x and W
 * for the forward, dy and W for the data gradient.  Nothing else changes: the weight and bias gradients dW = dy^T x, db are
 * formed in exact fp32 from the unrounded dy and x (their reduction runs over the rows and has 9-36 output tiles: it would
 * need a split-K bf16 kernel), every kept activation, the parameters, gradients and optimizer state, LayerNorm, LayerScale,
 * GELU, the attention products and the softmax, the loss, the patch embedding, the position table's resample and the token
 * assembly are fp32 as above.  A product of K terms then carries about 2^-9 sqrt(2) relative error per term instead of
 * 2^-24: gradients agree with float64 to some 1e-2 relative L2 per tensor instead of 1e-5.  The default is exact fp32.
 *
 * gemm_mode 3 (bit 0: the bf16 GEMMs of mode 1, bit 1: bf16 attention) is mode 1 plus a block's attention as a bf16-operand, fp32-accumulate flash attention (csrc/dvt_s3_attn.hip):
 * q log2(e) / 8, k and v are rounded once to bf16, P is rounded for P v; the forward keeps ao in fp32 and one fp32 log-sum-exp
 * per query row, no probabilities; the backward recomputes P = 2^(s - lse) per tile and forms dv = P^T dao, dS = P (.) (dao v^T
 * - D), dq = dS k / 8, dk = dS^T q / 8 with dao, P and dS rounded to bf16 as operands and D = dao . ao in fp32.  No float
 * atomics.  The k third of a qkv bias gradient, which is identically zero (a softmax row ignores a common shift of its logits) and
 * would otherwise receive the rounding residue of dS, is not accumulated: mode 3 adds nothing to it.  Neither P nor a block's fp32 qkv is kept (ViT-B/14 at 518 x 518: 95 MB + 13 MB per image and block less, 6.5 MB of
 * bf16 operands more).  Everything else -- the teacher, parameters, gradients, AdamW state, checkpoints, LayerNorm,
 * LayerScale, GELU, the loss, the weight gradients, the patch embedding and the position resample -- is as in mode 1.
 *
 * gemm_modes 5 and 7 (bit 4 on top of mode 1 resp. 3: bf16 weight gradients) form the weight gradient of a block's four linear
 * layers as dW[n][k] += sum_r bf16(dy[r][n]) bf16(x[r][k]) on v_mfma_f32_32x32x16_bf16 with fp32 accumulation
 * (csrc/dvt_s3_wgrad.hip): dy's rounding is the one the data gradient of the same layer already uses, x is rounded by one more row
 * cast.  The reduction over the token rows is split into S chunks of whole 64-row steps, each (128 x 128 tile, chunk) workgroup
 * writes an fp32 partial tile and a second pass adds the S partials in ascending chunk order into dW: no float atomics, two runs
 * give the same bits.  S = min(ceil(1024 / tiles), R / 256), at least 1, tiles = (n / 128) (k / 128): a function of (R, n, k) alone.
 * What stays fp32: every bias gradient db = colsum(dy) from the unrounded dy (mode 7 drops the k third of the qkv bias gradient
 * exactly as mode 3), the patch embedding's weight gradient (k_patch is not on the 128 grid), and everything modes 1 and 3 keep.
 *
 * Conventions as in dvt_hip.h: int return codes (0 = ok, DVT_E_* / hipError_t otherwise), device pointers owned by the
 * caller, `stream` is a hipStream_t, nothing synchronises.
 */
#ifndef DVT_STAGE3_H
#define DVT_STAGE3_H

#include <stdint.h>

#include "dvt_vit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DVT_S3_TENSORS_PER_BLOCK 14

/* Arena layout (floats; every slice starts on a 16-byte boundary, tensors keep the timm shapes):
 *   out[0] patch_embed.proj.weight [dim, 3, patch, patch]   out[1] patch_embed.proj.bias [dim]
 *   out[2] cls_token [1, 1, dim]   out[3] reg_token [1, n_prefix - 1, dim] (empty without registers; it follows cls_token
 *          directly, so the prefix tokens are one [n_prefix, dim] matrix)   out[4] pos_embed [1, pos_has_cls + gh gw, dim]
 *   out[5 + 14 b + i], block b, i = norm1.weight, norm1.bias, attn.qkv.weight [3 dim, dim], attn.qkv.bias,
 *          attn.proj.weight [dim, dim], attn.proj.bias, ls1.gamma, norm2.weight, norm2.bias, mlp.fc1.weight [mlp, dim],
 *          mlp.fc1.bias, mlp.fc2.weight [dim, mlp], mlp.fc2.bias, ls2.gamma
 *   out[5 + 14 depth] norm.weight, out[6 + 14 depth] norm.bias, out[7 + 14 depth] = total floats (a multiple of 4).
 * `out` must hold 8 + 14 depth entries.  dvt_s3_param_offsets_pos keeps pos_embed at the checkpoint's grid instead. */
int dvt_s3_param_offsets(const DvtVitConfig* cfg, int64_t* out);

/* Bytes of scratch for a step over `batch` images (every block's activations are kept). */
int64_t dvt_s3_workspace_bytes(const DvtVitConfig* cfg, int batch);

/* One step: forward, loss on the patch rows, backward.  img [batch, 3, img_h, img_w] fp32 (normalised), target
 * [batch, grid_h, grid_w, dim] fp32.  Gradients are ACCUMULATED into `grads` (layout of `params`); the image gets none.
 * loss_out: device float[4] = {loss, l2_loss, cosine_similarity_loss, 0} (overwritten).  feat_out may be NULL, else it
 * receives the student features [batch, grid_h, grid_w, dim]. */
int dvt_s3_train_step(const DvtVitConfig* cfg, const float* params, float* grads, const float* img, const float* target,
                      float* feat_out, int batch, void* work, int64_t work_bytes, float* loss_out, void* stream);

/* The same step over a slice of `batch` images of a batch of `norm_batch` (>= batch): the loss terms are normalised by the
 * whole batch, so the gradients of the slices add up to the gradient of the whole batch.  loss_out = {l2 + c, l2, c, 0}
 * with l2 = this slice's part of the whole batch's l2_loss and 1 - c its part of the mean cosine similarity: over the
 * slices, l2_loss = sum l2, cosine_similarity_loss = 1 - sum (1 - c).  norm_batch == batch is dvt_s3_train_step. */
int dvt_s3_train_slice(const DvtVitConfig* cfg, const float* params, float* grads, const float* img, const float* target,
                       float* feat_out, int batch, int norm_batch, void* work, int64_t work_bytes, float* loss_out,
                       void* stream);

/* ---- a position table at another grid than the run's -------------------------------------------------------------
 * timm (dynamic_img_size) resamples pos_embed in every forward -- F.interpolate(bicubic, antialias, align_corners=False) in
 * fp32 on the square g0 x g0 patch part of the table, prefix rows carried over -- and autograd carries the gradient back to
 * the checkpoint's table.  The map is linear and separable: per channel O = Wy P Wx^T.  The caller supplies the two tables,
 * dense, on the device: wy [grid_h, g0], wx [grid_w, g0] (row = output position; taken from torch itself by
 * dvt_amd.s3.pos_tables).  A table may be NULL when its axis keeps its length (g0 == grid_h resp. grid_w): the identity.
 * Entries that are exactly zero are skipped and the remaining taps are summed in ascending order, one fma each: no atomics,
 * no shared memory, two runs give the same bits.  dim % 4 == 0, every pointer 16-byte aligned.
 *
 * Forward: pos [has_cls + g0 g0, dim] -> out [has_cls + grid_h grid_w, dim]; x pass T[p, j] = sum_q wx[j, q] P[p, q] into
 * tmp [g0, grid_w, dim], then y pass O[i, j] = sum_p wy[i, p] T[p, j] (ATen's order); the cls row is copied. */
int dvt_pos_resample_fwd(const float* pos, float* out, const float* wy, const float* wx, float* tmp, int g0, int grid_h,
                         int grid_w, int dim, int has_cls, void* stream);

/* Transpose: dout [has_cls + grid_h grid_w, dim] -> dpos [has_cls + g0 g0, dim], ACCUMULATED:
 * dT[p, j] = sum_i wy[i, p] dO[i, j] into tmp [g0, grid_w, dim], then dP[p, q] += sum_j wx[j, q] dT[p, j]; the cls row's
 * gradient is added straight through. */
int dvt_pos_resample_bwd(const float* dout, float* dpos, const float* wy, const float* wx, float* tmp, int g0, int grid_h,
                         int grid_w, int dim, int has_cls, void* stream);

/* The step with pos_embed kept at the CHECKPOINT's shape [1, pos_has_cls + g0 g0, dim] in all four arenas: the layout of
 * dvt_s3_param_offsets with out[4] sized for g0 x g0 (g0 >= 1, else DVT_E_BADARG). */
int dvt_s3_param_offsets_pos(const DvtVitConfig* cfg, int g0, int64_t* out);

/* dvt_s3_workspace_bytes plus, when g0 x g0 is not the run's grid, the run-grid table, its gradient and the resample's
 * intermediate.  -1 for g0 < 1. */
int64_t dvt_s3_workspace_bytes_pos(const DvtVitConfig* cfg, int batch, int g0);

/* dvt_s3_train_slice over that layout.  When g0 x g0 is the run's grid the tables are ignored and the call IS
 * dvt_s3_train_slice.  Otherwise each call resamples `params`' table into the workspace for the token assembly, lets the
 * assembly's backward add into a zeroed run-grid gradient there, and adds its transpose into `grads` (slices stay additive:
 * the map is linear).  DVT_E_BADARG, before any pointer is touched: g0 < 1, a NULL table on an axis whose length is not g0,
 * a workspace below dvt_s3_workspace_bytes_pos. */
int dvt_s3_train_slice_pos(const DvtVitConfig* cfg, int g0, const float* wy, const float* wx, const float* params,
                           float* grads, const float* img, const float* target, float* feat_out, int batch, int norm_batch,
                           void* work, int64_t work_bytes, float* loss_out, void* stream);

/* ---- opt-in mixed precision (see "Arithmetic" at the top) -------------------------------------------------------------
 * gemm_mode: 0 = exact fp32 (the call IS dvt_s3_train_slice_pos -- dvt_s3_train_slice for g0 = 0 -- and the workspace theirs),
 *            1 = bf16 operands in the forward and data-gradient GEMMs of qkv / proj / fc1 / fc2, everything else as in 0,
 *            3 = mode 1 and the bf16 flash attention (its workspace: mode 1's less every block's P, the dP scratch and every
 *                block's fp32 qkv, plus 6 dim + 4 heads bytes per token row and block and 12 dim bytes).  The value is a bit set -- 1: the bf16
 *                GEMMs, 2: the bf16 attention -- and the attention is built on the GEMM mode: 2 alone is refused.
 *            5 = mode 1 and 7 = mode 3 with bit 4, the bf16 split-K weight gradients; built on the GEMM mode too: 4 and 6 are
 *                refused.  Their workspace is mode 1's resp. 3's, byte for byte, and BEHIND it two pieces (each rounded up to 256
 *                bytes): 2 max(mlp_dim, dim) bytes per token row (the layer input's row cast) and the partial tiles of the
 *                largest layer, max over qkv / proj / fc1 / fc2 of dvt_s3_wgrad_bf16_scratch_bytes' last two terms below,
 *                4 S n k + 4 Sb n bytes, one buffer for all layers and blocks.
 * Modes 1 and 3 round the four weights of every block once per call into the workspace (as stored for the forward, transposed for
 * the data gradient: params change between steps, and each slice rounds the same weights, so slices stay additive) and each
 * A operand into one shared scratch right before its GEMM; the workspace grows by 4 bytes per block weight and
 * 2 max(mlp_dim, 3 dim) bytes per token row, behind mode 0's carving.  g0 as for the _pos calls, or 0: the table is at the
 * run's grid, the layout of dvt_s3_param_offsets and the step of dvt_s3_train_slice (wy, wx ignored).  DVT_E_BADARG (-1 for the
 * size) before any launch: another gemm_mode, g0 < 0, a workspace below the mode's
 * size, a null pointer, in modes 1, 3, 5 and 7 `params` or `work` not 16-byte aligned. */
int64_t dvt_s3_workspace_bytes_mp(const DvtVitConfig* cfg, int batch, int g0, int gemm_mode);
int dvt_s3_train_slice_pos_mp(const DvtVitConfig* cfg, int g0, const float* wy, const float* wx, int gemm_mode,
                              const float* params, float* grads, const float* img, const float* target, float* feat_out,
                              int batch, int norm_batch, void* work, int64_t work_bytes, float* loss_out, void* stream);

/* The mode's casts, exported for tests (csrc/dvt_s3_cast.hip).  Round to nearest even on the bit pattern, as torch's
 * .to(torch.bfloat16): denormals and the sign of zero are kept, a finite value beyond the bf16 range becomes infinity.
 *   dvt_s3_cast_bf16:   x fp32 [rows, n] -> y bf16 [rows, n];  n % 4 == 0.
 *   dvt_s3_cast_bf16_t: w fp32 [n, k]    -> wt bf16 [k, n] (the transpose);  n % 64 == k % 64 == 0.
 * Pointers 16-byte aligned; DVT_E_BADARG otherwise, nothing launched. */
int dvt_s3_cast_bf16(const float* x, void* y, int64_t rows, int n, void* stream);
int dvt_s3_cast_bf16_t(const float* w, void* wt, int n, int k, void* stream);

/* The weight gradient of gemm_modes 5 and 7, exported for tests (csrc/dvt_s3_wgrad.hip):
 *   dw[n][k] (+)= sum_r bf16(dy[r][n]) bf16(x[r][k]) (fp32 accumulation),  db[n] (+)= sum_r dy[r][n] (dy unrounded)
 * dy fp32 [R, n], x fp32 [R, k]; R, n, k multiples of 128.  splits: 0 = the rule of "Arithmetic" above, >= 1 forces S (clamped
 * to the R / 64 row steps).  accumulate: 0 overwrites dw and db, 1 adds to them.  The call rounds dy and x into `scratch`
 * (dvt_s3_cast_bf16) itself.  scratch bytes, each term rounded up to 256: 2 R n + 2 R k + 4 S n k + 4 Sb n with Sb = clamp(R /
 * 1024, 1, 128) chunks of the column sum.  No float atomics: two runs give the same bits.
 * DVT_E_BADARG (-1 for the size), nothing launched: a null pointer, a shape off that grid, dy / x / dw / db / scratch not
 * 16-byte aligned, scratch_bytes below the size, splits < 0. */
int64_t dvt_s3_wgrad_bf16_scratch_bytes(int64_t R, int n, int k, int splits);
int dvt_s3_wgrad_bf16(const float* dy, const float* x, float* dw, float* db, void* scratch, int64_t scratch_bytes, int64_t R, int n,
                      int k, int splits, int accumulate, void* stream);

/* gemm_mode 3's attention, exported for tests (csrc/dvt_s3_attn.hip).  Head dimension 64, C = 64 heads, R = batch Tp token rows
 * of which the first T of every image are valid; keys >= T are masked.  No float atomics: two runs give the same bits.
 *   dvt_s3_attn_fwd: qkv fp32 [R, 3 C] (q | k | v) -> qkvb, the bf16 operands the backward reads again
 *       ([3][batch heads][Tp][64]: q log2(e) / 8, k, v, each rounded once; dvt_s3_attn_operand_bytes bytes),
 *       ao fp32 [R, C] = softmax(q k^T / 8) v and lse fp32 [batch heads, Tp] = log2 sum_k 2^(q' . k), q' the rounded scaled q.
 *       Rows t >= T: ao = 0, lse = 0.
 *   dvt_s3_attn_bwd: dao = d ao fp32 [R, C] -> dqkv fp32 [R, 3 C] (dq | dk | dv), every element written, rows t >= T zero;
 *       D [batch heads, Tp] is scratch (it receives rowsum(dao (.) ao)).  P = 2^(q' . k - lse) is recomputed.
 * DVT_E_BADARG, nothing launched: a null pointer, batch or heads < 1, Tp % 128 != 0, T < 1, T > Tp, qkv / qkvb / ao / dao /
 * dqkv not 16-byte aligned, more than 2^31 - 1 elements in qkv. */
int64_t dvt_s3_attn_operand_bytes(int batch, int heads, int Tp);
int dvt_s3_attn_fwd(const float* qkv, void* qkvb, float* ao, float* lse, int batch, int heads, int T, int Tp, void* stream);
int dvt_s3_attn_bwd(const void* qkvb, const float* ao, const float* dao, const float* lse, float* D, float* dqkv, int batch,
                    int heads, int T, int Tp, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DVT_STAGE3_H */
