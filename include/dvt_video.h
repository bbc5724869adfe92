/*
 * dvt_video.h -- C ABI of the feature-video demo in libdvt_hip.so (gfx950).
 *
 * Replaces the per-frame arithmetic of the reference's make_video_demo.py after the extractor: bases, k-means centres and
 * foreground bases are fitted ONCE (on frame 0, with the functions of dvt_vis.h) and here only APPLIED to every frame;
 * every map is min-max normalised per frame, turned into a token-resolution uint8 picture and upsampled with Pillow's
 * 8-bit bicubic filter.
 *
 * Data: features fp32 row-major [n, C] as in dvt_vis.h (C % 64 == 0, 64 <= C <= DVT_VIS_MAX_C, 1 <= n <= DVT_VIS_MAX_ROWS,
 * 16-byte aligned).  Projections P are fp32 row-major [n, m], 1 <= m <= DVT_VIDEO_MAX_M.  Pictures are uint8 [h, w, 3].
 *
 * Arithmetic: row-wise dot products (projections, norms, cosines) accumulate in fp64 and round once; the softmax sum is fp64;
 * everything else is single fp32 operations that are never contracted into FMAs, so that numpy's float32 arithmetic on the
 * same inputs gives the same bits.  Reductions run in a fixed order, there are no floating-point atomics and no function
 * needs scratch memory.  An affine image of a column is fl(fl(s * v) + o) (s = -1, o = 1: the script's `1 - v`).
 *
 * Conventions as in dvt_hip.h: int return codes (0 = ok, DVT_E_* / hipError_t otherwise), device pointers owned by the
 * caller, `stream` is a hipStream_t, nothing synchronises.  A call that returns DVT_E_BADARG has written nothing.
 */
#ifndef DVT_VIDEO_H
#define DVT_VIDEO_H

#include <stdint.h>

#include "dvt_vis.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DVT_VIDEO_MAX_M 32       /* columns of one apply */
#define DVT_VIDEO_MAX_TAPS 64    /* filter taps per output index of the resize */
#define DVT_VIDEO_MAX_IMAGES 64  /* pictures of one resize call */

/* One pass over x [n, C]: P [n, m] = x M (M fp32 [C, m] row-major), norms [n] = |x_i| (NULL: not written) and, with
 * centers [K, C] (centers and labels both or neither; 1 <= K <= DVT_VIS_MAX_K), labels [n] = the centre of largest cosine
 * similarity by the rule of dvt_vis_kmeans (lowest index on a tie, a zero row or centre has similarity 0). */
int dvt_video_apply(const float* x, int n, int C, const float* M, int m, const float* centers, int K, float* P, float* norms,
                    int32_t* labels, void* stream);

/* range fp32 [2, m] = the minimum (row 0) and maximum (row 1) of every column of P [n, m]; with affine_col >= 0 also
 * affine_range fp32 [2] = minimum and maximum of s * P[:, affine_col] + o.  affine_col < 0: affine_range is not touched. */
int dvt_video_col_range(const float* P, int n, int m, float* range, int affine_col, float s, float o, float* affine_range,
                        void* stream);

/* out [n] = softmax(norms / temp) over all n values (maximum subtracted, fp64 exponentials and sum, rounded to fp32), then
 * (p - min p) / (max p - min p) in fp32; a zero range gives what fp32 division gives (NaN). */
int dvt_video_softmax_norm_map(const float* norms, int n, float temp, float* out, void* stream);

/* mask [n] = (s * P[:, col] + o > t) as 0 / 1. */
int dvt_video_threshold_mask(const float* P, int n, int m, int col, float s, float o, float t, uint8_t* mask, void* stream);

/* ---- token-resolution pictures, uint8 [n, 3] (n = h w); a value v becomes (uint8) (v * 255) truncated, as
 * (v * 255).astype(np.uint8) does on a float32 array (NaN and negative values: 0, above 255: 255) --------------------- */

/* Three columns col0 .. col0 + 2 of P, each (v - min) / (max - min) with range [2, m] from dvt_video_col_range, times
 * mask [n] (0 / 1; NULL: none). */
int dvt_video_picture_rgb(const float* P, int n, int m, int col0, const float* range, const uint8_t* mask, uint8_t* out,
                          void* stream);

/* One value per row, v[i * stride + col], optionally s * v + o (affine != 0), optionally (v - lo) / (hi - lo) with lo =
 * range[0], hi = range[range_stride] (a column of a dvt_video_col_range result: its address and m; its affine_range: 1;
 * range NULL: v is used as it is), coloured by table uint8 [256, 3] at min(int(v * 256), 255):
 * what a matplotlib colour map returns for a float, already converted to uint8 by the caller.  NaN: black. */
int dvt_video_picture_scalar(const float* v, int n, int stride, int col, int affine, float s, float o, const float* range,
                             int range_stride, const uint8_t* table, uint8_t* out, void* stream);

/* Labels int32 [n] through table uint8 [K, 3]; a label outside [0, K) gives black. */
int dvt_video_picture_labels(const int32_t* labels, int n, const uint8_t* table, int K, uint8_t* out, void* stream);

/* out uint8 [H, W, 3] from a normalised image img fp32 [3, H, W]: v = (img - mean[c]) / std[c] (the script's denormalizer,
 * mean / std fp32 [3] on the device), clamped to [0, 1], times 255, truncated. */
int dvt_video_denorm_u8(const float* img, int H, int W, const float* mean, const float* std, uint8_t* out, void* stream);

/* images pictures src uint8 [images, h, w, 3] -> dst uint8 [images, H, W, 3], bit-identical to Pillow's
 * Image.resize((W, H), Image.BICUBIC) of 8-bit images: a horizontal pass into tmp uint8 [images, h, W, 3], then a vertical
 * pass, both in 32-bit integer arithmetic: acc = 2^21 + sum_t src[first + t] * coef[t], acc >> 22, clamped to [0, 255].
 * The caller computes Pillow's tables in float64 and uploads them: xbounds int32 [W, 2] = (first source column, taps),
 * xcoef int32 [W, xtaps]; ybounds int32 [H, 2], ycoef int32 [H, ytaps] likewise for rows.  The host cannot see the device
 * tables, so the kernels clamp every tap to the source (a wrong table gives a wrong picture, never a wild read). */
int dvt_video_resize_bicubic_u8(const uint8_t* src, int images, int h, int w, uint8_t* dst, int H, int W,
                                const int32_t* xbounds, const int32_t* xcoef, int xtaps, const int32_t* ybounds,
                                const int32_t* ycoef, int ytaps, uint8_t* tmp, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DVT_VIDEO_H */
