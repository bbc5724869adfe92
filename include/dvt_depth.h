/*
 * dvt_depth.h -- C ABI of the linear-probe depth evaluation in libdvt_hip.so (gfx950).
 *
 * Replaces, for the reference's `evaluate_dense_tasks.py --task depth` with the NYU linear config, the decode head its
 * evaluation/depth builds (`BNHead` with norm_cfg=None: the cls token broadcast behind the patch channels, a bilinear
 * upsample by `up`, `conv_depth` = a 1 x 1 convolution 2C -> K bins, p = relu(z) + 0.1 normalised over the bins, depth =
 * sum_k p_k bin_k), its losses (the prediction resized to the ground truth, SigLoss with warm-up, and GradientLoss as the
 * reference's indexing really computes it: differences between images j and j + 2 of the batch sub-sampled by 1, 2, 4 and
 * 6, zero for a batch below 3), gradient clipping, and the evaluation (flip average, clamp, resize, nine metrics).
 *
 * The convolution commutes with the upsample (bilinear weights sum to one), so the logits are computed at token
 * resolution: Z [B h w, K] = X W[:, :C]^T + (cls W[:, C:]^T + b), and interpolated per output pixel.
 *
 * Data: features NHWC fp32 [batch, h, w, C], cls fp32 [batch, C], ground truth fp32 [batch, H, W] (<= 0 or NaN = invalid),
 * bins fp32 [K] (the caller's linspace).  C % 64 == 0, K % 4 == 0, 4 <= K <= 256, 1 <= up <= 8, batch <= 64.
 *
 * Arithmetic: exact fp32 for the head, its loss and every gradient; the scalar statistics of the loss (merging the
 * per-block count / mean / M2 records by Chan's rule) and the metric sums run in fp64.  Every reduction runs in a fixed
 * order, there are no atomics, and a workspace filled with anything (NaN included) gives the same bits.
 *
 * Conventions as in dvt_hip.h: int return codes (0 = ok, DVT_E_* / hipError_t otherwise), device pointers owned by the
 * caller, `stream` is a hipStream_t, nothing synchronises.
 */
#ifndef DVT_DEPTH_H
#define DVT_DEPTH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVT_DEPTH_MAX_BINS 256
#define DVT_DEPTH_MAX_BATCH 64
#define DVT_DEPTH_MAX_UP 8

/* Parameter arena (floats): out[0] conv_depth.weight [K, 2C] (patch channels, then cls channels), out[1] conv_depth.bias
 * [K], out[2] = total floats.  Gradients and AdamW moments share the layout, so dvt_adamw_step (dvt_stage2.h) steps it. */
int dvt_depth_param_offsets(int C, int K, int64_t* out);

/* Bytes of scratch for dvt_depth_train_step / dvt_depth_forward (gt_h = gt_w = 0: the forward alone). */
int64_t dvt_depth_workspace_bytes(int batch, int h, int w, int C, int K, int up, int gt_h, int gt_w);

/* The head: depth [batch, up h, up w]. */
int dvt_depth_forward(const float* params, const float* bins, const float* x, const float* cls, int batch, int h, int w,
                      int C, int K, int up, float* depth, void* work, int64_t work_bytes, void* stream);

/* One training step of the head: forward, both losses against gt [batch, gt_h, gt_w], and the gradients of the
 * parameter arena (written, not accumulated).  warm_up != 0: SigLoss's warm-up form sqrt(0.15 mean(g)^2).
 * out: device float[2] = {loss_depth, grad_weight * gradient loss}.  Without a valid pixel (or, after the warm-up, with
 * fewer than two) loss_depth is NaN and every gradient is written as 0.  A sub-sampled batch of the gradient loss
 * without a valid pixel contributes 0 (the reference: 0 / 0). */
int dvt_depth_train_step(const float* params, float* grads, const float* bins, const float* x, const float* cls,
                         const float* gt, int batch, int h, int w, int C, int K, int up, int gt_h, int gt_w,
                         int warm_up, float grad_weight, void* work, int64_t work_bytes, float* out, void* stream);

/* torch.nn.utils.clip_grad_norm_ on the device: norm = the L2 norm of grads [n] in a fixed order, then grads *=
 * min(1, max_norm / (norm + 1e-6)).  work: at least dvt_depth_clip_work_floats(n) floats; out: device float[2] =
 * {norm, factor}. */
int64_t dvt_depth_clip_work_floats(int64_t n);
int dvt_depth_clip_grad_norm(float* grads, int64_t n, float max_norm, float* work, float* out, void* stream);

/* Evaluation of one image.  d0 [uh, uw]: the head's depth of the image, d1 (may be NULL): that of its horizontal flip.
 * Each is clamped to [min_depth, max_depth] and resized (bilinear, align_corners=False) to out_h x out_w, d1 is flipped
 * back, and the two are averaged into pred (fp32 [out_h, out_w], may be NULL).  Over the pixels with min_depth < gt <
 * max_depth inside rows [crop_y0, crop_y1) and columns [crop_x0, crop_x1): row [9] (fp64) = a1, a2, a3, abs_rel, rmse,
 * log_10, rmse_log, silog, sq_rel; all NaN without such a pixel, silog 0 where its root is NaN.
 * work: at least dvt_depth_eval_work_bytes(out_h, out_w) bytes. */
int64_t dvt_depth_eval_work_bytes(int out_h, int out_w);
int dvt_depth_eval_image(const float* d0, const float* d1, int uh, int uw, const float* gt, int out_h, int out_w,
                         float min_depth, float max_depth, int crop_y0, int crop_y1, int crop_x0, int crop_x1,
                         float* pred, double* row, void* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DVT_DEPTH_H */
