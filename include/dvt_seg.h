/*
 * dvt_seg.h -- C ABI of the linear-probe segmentation evaluation in libdvt_hip.so (gfx950).
 *
 * Replaces, for the reference's `evaluate_dense_tasks.py --task segmentation` with the linear configs, the decode head
 * mmseg 0.27 builds there (`BNHead`: SyncBatchNorm over the frozen backbone features, then `conv_seg`, a 1 x 1 convolution
 * to K classes), its loss (bilinear resize of the logits to the label size, align_corners=False, then CrossEntropyLoss with
 * ignore_index 255 averaged over ALL label pixels, avg_non_ignore=False), and the evaluation (EncoderDecoder.slide_inference,
 * the resize to the original image, argmax, intersect_and_union histograms).
 *
 * Data: features are NHWC fp32 [batch, h, w, C] as the extractor writes them, n_rows = batch h w; labels are uint8
 * [batch, label_h, label_w] (255 = ignore).  C % 64 == 0 (384 / 768 / 1024), 1 <= K <= 256.
 *
 * Arithmetic: exact fp32.  Every reduction runs in a fixed order (no float atomics), so results do not depend on timing,
 * and a workspace filled with anything (NaN included) gives the same bits.  The only atomics are the integer histogram
 * adds of dvt_seg_finalize.
 *
 * Statistics records: a record is DVT_SEG_STATS_FLOATS(C) = 3 C + 4 floats: mean_hi[C], mean_lo[C] (the mean is the
 * fp32 pair hi + lo), M2[C] (sum of squared deviations), count, 0, 0, 0.  Records merge by Chan's rule, so per-rank
 * records of a data-parallel run can be gathered and merged (SyncBN) before the step normalises.
 *
 * Conventions as in dvt_hip.h: int return codes (0 = ok, DVT_E_* / hipError_t otherwise), device pointers owned by the
 * caller, `stream` is a hipStream_t, nothing synchronises.
 */
#ifndef DVT_SEG_H
#define DVT_SEG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVT_SEG_STATS_FLOATS(C) (3 * (C) + 4)
#define DVT_SEG_MAX_CLASSES 256

/* Parameter arena (floats, every slice 4-aligned): out[0] conv_seg.weight [K, C], out[1] conv_seg.bias [K],
 * out[2] bn.weight [C], out[3] bn.bias [C], out[4] = total floats.  Gradients and AdamW moments share the layout, so
 * dvt_adamw_step (dvt_stage2.h) steps the head.  Running statistics live apart: running[0:C] mean, running[C:2C] var. */
int dvt_seg_param_offsets(int C, int K, int64_t* out);

/* Statistics records written by dvt_seg_bn_stats for n_rows rows (one record per block of 128 rows). */
int dvt_seg_stats_parts(int64_t n_rows);

/* Bytes of scratch for dvt_seg_train_step / dvt_seg_forward. */
int64_t dvt_seg_workspace_bytes(int batch, int h, int w, int C, int K, int label_h, int label_w);

/* Per-channel statistics of x [n_rows, C]: `parts` receives dvt_seg_stats_parts(n_rows) records (within a
 * block of rows, sums shifted by its first row), `stats` one record, their merge in block order. */
int dvt_seg_bn_stats(const float* x, int64_t n_rows, int C, float* parts, float* stats, void* stream);

/* Merge n_parts records (e.g. one per rank) in order into `stats`. */
int dvt_seg_bn_merge(const float* parts, int n_parts, int C, float* stats, void* stream);

/* One training step of the head.  stats: the record to normalise with (the merged record of every rank under SyncBN),
 * or NULL for this batch's own.  Writes (does not accumulate) the gradients of the parameter arena; updates `running`
 * (momentum, running_var from the unbiased variance); out: device float[2] = {loss, acc_seg in percent}.  The caller
 * counts num_batches_tracked. */
int dvt_seg_train_step(const float* params, float* grads, float* running, const float* x, const uint8_t* labels,
                       const float* stats, int batch, int h, int w, int C, int K, int label_h, int label_w,
                       float momentum, float eps, void* work, int64_t work_bytes, float* out, void* stream);

/* Inference head: z [n_rows, K] = conv_seg(BN(x)) with the running statistics. */
int dvt_seg_forward(const float* params, const float* running, const float* x, int64_t n_rows, int C, int K,
                    float eps, float* z, void* work, int64_t work_bytes, void* stream);

/* Slide inference, one crop: the crop's logits z [h, w, K] resized (bilinear, align_corners=False) to crop_h x crop_w are
 * added into canvas [K, H, W] at (y0, x0), and count [H, W] += 1 there.  Crops are added in launch order. */
int dvt_seg_slide_accum(const float* z, int h, int w, int K, int crop_h, int crop_w, int y0, int x0, float* canvas,
                        float* count, int H, int W, void* stream);

/* Per output pixel of out_h x out_w: canvas / count resized (bilinear, align_corners=False) to the output size, argmax
 * over the K classes (first maximum), then intersect_and_union against label [out_h, out_w] (uint8; reduce_zero_label:
 * 0 -> 255, l -> l - 1).  hist [3, K] int64 += area_intersect, area_pred, area_label.  pred (int32 [out_h, out_w]) may
 * be NULL. */
int dvt_seg_finalize(const float* canvas, const float* count, int K, int H, int W, const uint8_t* label, int out_h,
                     int out_w, int reduce_zero_label, int64_t* hist, int32_t* pred, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DVT_SEG_H */
