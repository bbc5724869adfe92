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
 * Arithmetic: exact fp32 throughout, on the kernels of the stage-2 step (csrc/dvt_s2_parts.h): linear layers on the
 * 128 x 128 x 32 exact-fp32 MFMA tile, the softmax fused into the two [s_pad][s_pad] attention products, probabilities kept
 * for the backward pass, two-pass LayerNorm statistics, erf GELU.  Every block keeps its activations: about 0.18 GB per image
 * and block for ViT-B/14 at 518 x 518 (host code splits a batch that does not fit into slices, dvt_s3_train_slice).
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

#ifdef __cplusplus
}
#endif
#endif /* DVT_STAGE3_H */
