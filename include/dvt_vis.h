/*
 * dvt_vis.h -- C ABI of the feature-map visualisation in libdvt_hip.so (gfx950).
 *
 * Replaces, for the tiled picture that the reference's main_img_denoising.py writes for every vis_freq-th image, the
 * arithmetic of its dvt/utils/visualization/visualization_tools.py: the robust PCA colours (get_robust_pca / get_pca_map),
 * the L2-norm map (get_scale_map), the centre-patch similarity map (get_similarity_map), the cosine k-means cluster map
 * (get_cluster_map) and the resampling, colour lookup and composition of the panels into one canvas.
 *
 * Data: features fp32 row-major [n, C] (a map [h, w, C] flattened), C % 64 == 0, 64 <= C <= DVT_VIS_MAX_C, 1 <= n <=
 * DVT_VIS_MAX_ROWS; x is 16-byte aligned (the covariance reads rows as float4; with C % 64 == 0 every row then is).  A row
 * mask is uint8 [n] (0 = row left out) or NULL (all rows).
 *
 * Arithmetic: exact fp32 (plain FMA) for the covariance and the orthogonal iteration; row-wise dot products (projections,
 * norms, cosines, k-means similarities and centre sums) accumulate in fp64 and round once; the column means, the median /
 * deviation selection and the k-means inertia run in fp64.  Every reduction runs in a fixed order,
 * there are no floating-point atomics (the radix select counts with integer LDS atomics, whose result does not depend on
 * their order), no workgroup ever waits for another one, and a workspace filled with anything (NaN included) gives the
 * same bits.
 *
 * Conventions as in dvt_hip.h: int return codes (0 = ok, DVT_E_* / hipError_t otherwise), device pointers owned by the
 * caller, `stream` is a hipStream_t, nothing synchronises.
 */
#ifndef DVT_VIS_H
#define DVT_VIS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVT_VIS_MAX_C 1024
#define DVT_VIS_MAX_ROWS 65536
#define DVT_VIS_MAX_K 16       /* clusters */
#define DVT_VIS_MAX_INIT 16    /* k-means restarts */
#define DVT_VIS_MAX_ITER 1000  /* Lloyd iterations, PCA iterations */

/* Bytes of scratch that every function below accepts for maps of up to n rows, C channels, K clusters and num_init
 * k-means restarts (K = num_init = 0: everything but dvt_vis_kmeans).  < 0: bad arguments. */
int64_t dvt_vis_workspace_bytes(int n, int C, int K, int num_init);

/* Top-3 principal directions of the rows with mask != 0 (mask NULL: all rows): column means, the C x C covariance
 * sum (x - mean)(x - mean)^T / (count - 1), then `iters` steps of orthogonal (block power) iteration on it from a fixed
 * dense start basis, modified Gram-Schmidt after every step.  Each direction has unit length and its largest-magnitude
 * component (lowest index on a tie) positive.  basis: fp32 [C, 3]; evals: fp32 [3], the Rayleigh quotients.  Fewer than
 * two rows selected: basis and evals are written as 0. */
int dvt_vis_pca_basis(const float* x, const uint8_t* mask, int n, int C, int iters, float* basis, float* evals,
                      void* work, int64_t work_bytes, void* stream);

/* out [n, 3] = x basis; with rgb_min / rgb_max (device fp32 [3], both or neither): clamp((x basis - min) / (max - min),
 * 0, 1), the reference's get_pca_map colours (a zero range gives what fp32 division gives; NaN is written as 0). */
int dvt_vis_project(const float* x, const float* basis, const float* rgb_min, const float* rgb_max, int n, int C,
                    float* out, void* stream);

/* The colour range of get_robust_pca from projected rows colors [n, 3], over the rows with mask != 0.  Per channel: med =
 * the median (the LOWER middle value for an even count), dev = the median of |c - med| (fp64), and the minimum / maximum of
 * c over the rows with |c - med| / dev < m.  If any channel has no such row (a zero deviation), ALL channels take the
 * reference's fall-back: the minimum / maximum over all rows (masked or not) and all three channels.
 *   range  fp32 [6]  = rgb_min[3], rgb_max[3]
 *   stats  fp64 [6]  = med[3], dev[3]
 *   rows   int32 [13] = the row (lowest index on a tie) that gave med[3], dev[3], min[3], max[3]; rows[12] = 1 on fall-back
 *                      (then min / max rows are those of the global extremes, repeated)
 * No row selected: everything NaN / -1.  stats and rows may be NULL. */
int dvt_vis_robust_range(const float* colors, const uint8_t* mask, int n, float m, float* range, double* stats,
                         int32_t* rows, void* work, int64_t work_bytes, void* stream);

/* mask_out [n] = ((colors[:, 0] - min) / (max - min) < thresh), min / max of channel 0 over all rows: the foreground mask
 * of get_robust_pca(remove_first_component=True). */
int dvt_vis_fg_mask(const float* colors, int n, float thresh, uint8_t* mask_out, void* stream);

/* out [n] = (|x_i| - min) / (max - min + 1e-6): get_scale_map before its colour table. */
int dvt_vis_norm_map(const float* x, int n, int C, float* out, void* work, int64_t work_bytes, void* stream);

/* out [h w] = cosine of every row with row (h / 2) * w + w / 2, min-max normalised, the centre itself set to -1:
 * get_similarity_map before its resampling. */
int dvt_vis_similarity_map(const float* x, int h, int w, int C, float* out, void* work, int64_t work_bytes, void* stream);

/* Cosine k-means (Lloyd).  Restart r starts from the rows init_rows[r, k] (int32 [num_init, K]) or, when init_centers is
 * not NULL, from the vectors init_centers [num_init, K, C].  One iteration: every row goes to the centre of largest
 * cosine similarity (lowest index on a tie; a zero vector has similarity 0), every centre becomes the mean of its rows
 * (an empty cluster keeps its centre), and the restart stops once the summed squared shift of its centres is below tol,
 * or after max_iter iterations.  The restart with the lowest inertia (sum over rows of 1 - similarity, fp64; lowest index
 * on a tie) wins.
 *   labels  int32 [n], inertia: the LAST assignment of the winning restart / of each restart
 *   centers fp32 [K, C]: the means of those labels
 *   inertia fp64 [num_init], iterations int32 [num_init] (== max_iter: the limit was reached), best int32 [1]
 * All 3 * max_iter + 4 launches are enqueued at once; a device-side flag turns those of a converged restart into no-ops.
 * 1 <= K <= DVT_VIS_MAX_K, K <= n, 1 <= num_init <= DVT_VIS_MAX_INIT, 1 <= max_iter <= DVT_VIS_MAX_ITER. */
int dvt_vis_kmeans(const float* x, int n, int C, int K, const int32_t* init_rows, const float* init_centers, int num_init,
                   int max_iter, float tol, int32_t* labels, float* centers, double* inertia, int32_t* iterations,
                   int32_t* best, void* work, int64_t work_bytes, void* stream);

/* ---- rendering into a caller-owned canvas fp32 [3, canvas_h, canvas_w] -------------------------------------------------
 * Every function writes the rectangle rows [y0, y0 + H), columns [x0, x0 + W); a rectangle that is empty or not inside the
 * canvas returns DVT_E_BADARG.  interp: 0 = nearest (source index min(floor(dst * (float) in / out), in - 1)), 1 =
 * bilinear with align_corners = False. */
#define DVT_VIS_NEAREST 0
#define DVT_VIS_BILINEAR 1

/* A scalar map [h, w], resampled; with table (device fp32 [256, 3]): colour = table[min(int(clamp(v, 0, 1) * 256), 255)],
 * without: grey.  neg_red != 0: a resampled value below 0 gives pure red (the similarity map's centre). */
int dvt_vis_render_scalar(const float* map, int h, int w, int interp, const float* table, int neg_red, float* canvas,
                          int canvas_h, int canvas_w, int y0, int x0, int H, int W, void* stream);

/* A colour map, [h, w, 3] (planar == 0) or [3, h, w] (planar != 0), resampled. */
int dvt_vis_render_rgb(const float* map, int h, int w, int planar, int interp, float* canvas, int canvas_h, int canvas_w,
                       int y0, int x0, int H, int W, void* stream);

/* Labels int32 [h, w] in [0, K), resampled (nearest), coloured by table (device fp32 [K, 3]); a label outside [0, K)
 * gives black. */
int dvt_vis_render_labels(const int32_t* labels, int h, int w, const float* table, int K, float* canvas, int canvas_h,
                          int canvas_w, int y0, int x0, int H, int W, void* stream);

/* One colour over the rectangle. */
int dvt_vis_fill(float* canvas, int canvas_h, int canvas_w, int y0, int x0, int H, int W, float r, float g, float b,
                 void* stream);

/* out uint8 [canvas_h, canvas_w, 3] = (uint8) (canvas * 255), truncated, after clamping to [0, 1] (NaN: 0). */
int dvt_vis_canvas_to_u8(const float* canvas, int canvas_h, int canvas_w, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DVT_VIS_H */
