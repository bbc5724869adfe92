// Linear-probe segmentation head and evaluation (include/dvt_seg.h): mmseg 0.27 BNHead + conv_seg + CrossEntropyLoss,
// slide inference and the intersect_and_union histograms, in exact fp32 with fixed-order reductions.
//
// Training step, per batch (no host synchronisation, nine launches):
//   seg_stats_kernel / seg_merge_kernel   shifted sums over blocks of 128 rows, Chan's rule over the blocks (SyncBN merges
//                                         the per-rank records with the same merge kernel)
//   seg_fold_kernel                       A = W diag(gamma / sigma), c = b + W beta; the running statistics update
//   seg_logits_kernel                     Z = (x - mu) A^T + c, a 64 x 64 fp32 tile (centring before the product, with
//                                         mu as an fp32 pair, keeps channels with large means from cancelling in the fold)
//   seg_loss_row_kernel                   one workgroup per label row: the bilinear upsample of Z, log-softmax, CE and
//                                         the softmax gradient per pixel, reduced along x into R [B, H, w, K]
//   seg_loss_finish_kernel                loss (mean over ALL label pixels), acc_seg
//   seg_dz_kernel                         the reduction of R along y: dZ [B, h, w, K]
//   seg_pgrad_partial_kernel              G_s = dZ_s^T x_hat and db_s over slabs of 256 rows
//   seg_pgrad_finish_kernel /
//   seg_pgrad_bn_kernel                   dW = G diag(gamma) + db beta^T, db, dgamma = sum_k W o G, dbeta = W^T db
//
// The bilinear source index and the two 64 x 64 tiles (logits, parameter-gradient slab) are dvt_head_dev.h's, shared with
// the depth head.
#include "dvt_head_dev.h"
#include "../../include/dvt_seg.h"

#include <float.h>

namespace {

constexpr int kStatRows = 128;  // rows per statistics record
constexpr int kSlab = 256;      // rows per parameter-gradient slab
constexpr int kChunk = 16;      // label pixels per chunk of the loss kernel

// ---------------------------------------------------------------------------------------------------- statistics
// A record holds the mean as an fp32 pair (hi + lo): one fp32 mean of a channel at 1e3 is off by up to 3e-5, which
// centring turns into an offset of every normalised value.  Within a block the sums are shifted by the block's first row
// (x - x0 is exact for values close together), so no sum cancels.
__global__ __launch_bounds__(256) void seg_stats_kernel(const float* __restrict__ x, int64_t n, int C,
                                                        float* __restrict__ parts) {
  const int64_t r0 = (int64_t)blockIdx.x * kStatRows;
  const int64_t r1 = min(n, r0 + kStatRows);
  float* rec = parts + (size_t)blockIdx.x * (3 * C + 4);
  const double cnt = (double)(r1 - r0);
  for (int c = threadIdx.x; c < C; c += 256) {
    const float x0 = x[r0 * C + c];
    float s1 = 0.f, s2 = 0.f;
    for (int64_t r = r0; r < r1; ++r) {
      const float d = x[r * C + c] - x0;
      s1 += d;
      s2 = fmaf(d, d, s2);
    }
    const double mean = (double)x0 + (double)s1 / cnt;
    const double m2 = (double)s2 - (double)s1 * (double)s1 / cnt;
    const float hi = (float)mean;
    rec[c] = hi;
    rec[C + c] = (float)(mean - (double)hi);
    rec[2 * C + c] = (float)(m2 > 0.0 ? m2 : 0.0);
  }
  if (threadIdx.x == 0) {
    rec[3 * C] = (float)(r1 - r0);
    rec[3 * C + 1] = rec[3 * C + 2] = rec[3 * C + 3] = 0.f;
  }
}

__global__ __launch_bounds__(256) void seg_merge_kernel(const float* __restrict__ parts, int n_parts, int C,
                                                        float* __restrict__ stats) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int stride = 3 * C + 4;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int p = 0; p < n_parts; ++p) {
    const float* rec = parts + (size_t)p * stride;
    const double nb = rec[3 * C];
    if (nb <= 0.0 || c >= C) {
      n += nb;
      continue;
    }
    const double mb = (double)rec[c] + (double)rec[C + c], m2b = rec[2 * C + c];
    const double tot = n + nb, d = mb - mean;
    mean += d * (nb / tot);
    m2 += m2b + d * d * (n * nb / tot);
    n = tot;
  }
  if (c < C) {
    const float hi = (float)mean;
    stats[c] = hi;
    stats[C + c] = (float)(mean - (double)hi);
    stats[2 * C + c] = (float)m2;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    stats[3 * C] = (float)n;
    stats[3 * C + 1] = stats[3 * C + 2] = stats[3 * C + 3] = 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------- BN fold
// folded: A [K, C], cvec [K], mean_hi [C], invstd [C], mean_lo [C].  Block k < K folds row k; block K writes mean / invstd and updates
// the running statistics (training).
__global__ __launch_bounds__(256) void seg_fold_kernel(const float* __restrict__ params, const float* __restrict__ stats,
                                                       float* __restrict__ running, int C, int K, int64_t off_b,
                                                       int64_t off_g, int64_t off_beta, int training, float momentum,
                                                       float eps, float* __restrict__ folded) {
  __shared__ float red[256];
  const float* W = params;
  const float* gamma = params + off_g;
  const float* beta = params + off_beta;
  const int k = blockIdx.x;
  const float cnt = training ? stats[3 * C] : 1.f;
  if (k == K) {
    for (int c = threadIdx.x; c < C; c += 256) {
      const float mu = training ? stats[c] : running[c];
      const float var = training ? stats[2 * C + c] / cnt : running[C + c];
      folded[(size_t)K * C + K + c] = mu;
      folded[(size_t)K * C + K + C + c] = 1.f / sqrtf(var + eps);
      const float mu_lo = training ? stats[C + c] : 0.f;
      folded[(size_t)K * C + K + 2 * C + c] = mu_lo;
      if (training) {
        const float unbiased = cnt > 1.f ? stats[2 * C + c] / (cnt - 1.f) : stats[2 * C + c];
        running[c] = (1.f - momentum) * running[c] + momentum * (mu + mu_lo);
        running[C + c] = (1.f - momentum) * running[C + c] + momentum * unbiased;
      }
    }
    return;
  }
  float acc = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float var = training ? stats[2 * C + c] / cnt : running[C + c];
    const float invstd = 1.f / sqrtf(var + eps);
    const float wkc = W[(size_t)k * C + c];
    folded[(size_t)k * C + c] = wkc * (gamma[c] * invstd);
    acc += wkc * beta[c];
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) folded[(size_t)K * C + k] = params[off_b + k] + red[0];
}

// ---------------------------------------------------------------------------------------------------- logits
// Z [n, K] = (x - mu) A^T + cvec.  Tile 64 rows x 64 classes, 32 channels per stage; thread (ty, tx) owns 4 x 4.
__global__ __launch_bounds__(256) void seg_logits_kernel(const float* __restrict__ x, int64_t n, int C, int K,
                                                         const float* __restrict__ folded, float* __restrict__ z) {
  const float* A = folded;
  const float* cvec = folded + (size_t)K * C;
  const float* mu = cvec + K;
  const float* mu_lo = mu + 2 * C;
  const int64_t n0 = (int64_t)blockIdx.x * 64;
  const int k0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc[4][4] = {};
  head_logits_tile(n0, n, k0, K, C, [&](int64_t row, int c) { return (x[row * C + c] - mu[c]) - mu_lo[c]; },
                   [&](int kk, int c) { return A[(size_t)kk * C + c]; }, acc);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = n0 + ty * 4 + i;
    if (row >= n) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kk = k0 + tx * 4 + j;
      if (kk < K) z[row * K + kk] = acc[i][j] + cvec[kk];
    }
  }
}

// ---------------------------------------------------------------------------------------------------- loss
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// One workgroup per label row (b, Y).  Pixels are taken kChunk at a time: each wave interpolates a pixel's K logits
// (lanes over classes), takes the log-softmax and writes the pixel's gradient row into LDS; then every (xs, k) of the
// row accumulator adds the chunk's pixels in x order.  rowpart[row] = {sum of CE, correct, valid pixels, 0}.
__global__ __launch_bounds__(256) void seg_loss_row_kernel(const float* __restrict__ z, const uint8_t* __restrict__ labels,
                                                           int h, int w, int K, int H, int W, float inv_total,
                                                           float* __restrict__ R, float* __restrict__ rowpart) {
  extern __shared__ float sm[];
  float* acc = sm;            // [w][K]
  float* g = sm + w * K;      // [kChunk][K]
  __shared__ int px0[kChunk], px1[kChunk], pvalid[kChunk];
  __shared__ float plx[kChunk];
  __shared__ float wred[4][3];
  const int row = blockIdx.x;
  const int b = row / H, Y = row - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Src sy = src_index(Y, h, (float)h / (float)H);
  const float sx_scale = (float)w / (float)W;
  const float* zb = z + (size_t)b * h * w * K;
  const float* z0 = zb + (size_t)sy.i0 * w * K;
  const float* z1 = zb + (size_t)sy.i1 * w * K;
  const uint8_t* lab = labels + (size_t)row * W;
  for (int i = threadIdx.x; i < w * K; i += 256) acc[i] = 0.f;
  float loss_w = 0.f, corr_w = 0.f, valid_w = 0.f;
  for (int X0 = 0; X0 < W; X0 += kChunk) {
    __syncthreads();
    for (int p = wave; p < kChunk; p += 4) {
      const int X = X0 + p;
      const int l = X < W ? (int)lab[X] : 255;
      if (l == 255 || l >= K) {  // ignored (or outside the classes): no loss, no gradient
        if (lane == 0) pvalid[p] = 0;
        continue;
      }
      const Src sx = src_index(X, w, sx_scale);
      float v[4];
      float m = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = lane + 64 * j;
        v[j] = -INFINITY;
        if (k < K) {
          const float top = sx.l0 * z0[(size_t)sx.i0 * K + k] + sx.l1 * z0[(size_t)sx.i1 * K + k];
          const float bot = sx.l0 * z1[(size_t)sx.i0 * K + k] + sx.l1 * z1[(size_t)sx.i1 * K + k];
          v[j] = sy.l0 * top + sy.l1 * bot;
          m = fmaxf(m, v[j]);
        }
      }
      m = wave_max(m);
      // first class reaching the maximum
      int best = 1 << 30;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = lane + 64 * j;
        if (k < K && v[j] == m && k < best) best = k;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
      float e[4], s = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        e[j] = (lane + 64 * j < K) ? expf(v[j] - m) : 0.f;
        s += e[j];
      }
      s = wave_sum(s);
      const int jl = l >> 6;
      const float vsel = jl == 0 ? v[0] : jl == 1 ? v[1] : jl == 2 ? v[2] : v[3];
      const float zl = __shfl(vsel, l & 63, 64);
      const float inv_s = 1.f / s;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = lane + 64 * j;
        if (k < K) g[p * K + k] = (e[j] * inv_s - (k == l ? 1.f : 0.f)) * inv_total;
      }
      if (lane == 0) {
        pvalid[p] = 1;
        px0[p] = sx.i0;
        px1[p] = sx.i1;
        plx[p] = sx.l1;
        loss_w += (m + logf(s)) - zl;
        corr_w += best == l ? 1.f : 0.f;
        valid_w += 1.f;
      }
    }
    __syncthreads();
    // pixels run in x order, so the chunk touches only the columns from its first valid pixel's x0 to its last one's x1
    int lo = w, hi = -1;
    for (int p = 0; p < kChunk; ++p)
      if (pvalid[p]) {
        lo = min(lo, px0[p]);
        hi = max(hi, px1[p]);
      }
    for (int i = lo * K + threadIdx.x; i < (hi + 1) * K; i += 256) {
      const int xs = i / K, k = i - xs * K;
      float a = acc[i];
      for (int p = 0; p < kChunk; ++p) {
        if (!pvalid[p]) continue;
        if (px0[p] == xs) a += (1.f - plx[p]) * g[p * K + k];
        if (px1[p] == xs) a += plx[p] * g[p * K + k];
      }
      acc[i] = a;
    }
  }
  __syncthreads();
  float* Rrow = R + (size_t)row * w * K;
  for (int i = threadIdx.x; i < w * K; i += 256) Rrow[i] = acc[i];
  if (lane == 0) {
    wred[wave][0] = loss_w;
    wred[wave][1] = corr_w;
    wred[wave][2] = valid_w;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* o = rowpart + (size_t)row * 4;
    o[0] = (wred[0][0] + wred[1][0]) + (wred[2][0] + wred[3][0]);
    o[1] = (wred[0][1] + wred[1][1]) + (wred[2][1] + wred[3][1]);
    o[2] = (wred[0][2] + wred[1][2]) + (wred[2][2] + wred[3][2]);
    o[3] = 0.f;
  }
}

// out = {sum CE / (B H W), acc_seg}: mmseg 0.27 accuracy(): (correct + eps) * 100 / (valid + eps), eps = FLT_EPSILON.
__global__ __launch_bounds__(256) void seg_loss_finish_kernel(const float* __restrict__ rowpart, int rows, float inv_total,
                                                              float* __restrict__ out) {
  __shared__ double red[3][256];
  double a = 0.0, c = 0.0, v = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) {
    a += rowpart[(size_t)r * 4];
    c += rowpart[(size_t)r * 4 + 1];
    v += rowpart[(size_t)r * 4 + 2];
  }
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = c;
  red[2][threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s)
      for (int q = 0; q < 3; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)(red[0][0] * (double)inv_total);
    const float ce = (float)red[1][0] + FLT_EPSILON;
    out[1] = ce * (float)(100.0 / (red[2][0] + (double)FLT_EPSILON));
  }
}

// dZ [b, ys, xs, k] = sum over label rows Y (in order) of the y weights of Y onto ys times R [b, Y, xs, k].
__global__ __launch_bounds__(256) void seg_dz_kernel(const float* __restrict__ R, int B, int h, int w, int K, int H,
                                                     float* __restrict__ dz) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)B * h * w * K;
  if (idx >= total) return;
  const int k = (int)(idx % K);
  int64_t t = idx / K;
  const int xs = (int)(t % w);
  t /= w;
  const int ys = (int)(t % h);
  const int b = (int)(t / h);
  const float scale = (float)h / (float)H;
  const int lo = max(0, (int)floorf(((float)ys - 0.5f) / scale - 0.5f) - 2);
  const int hi = min(H - 1, (int)ceilf(((float)ys + 1.5f) / scale - 0.5f) + 2);
  float a = 0.f;
  for (int Y = lo; Y <= hi; ++Y) {
    const Src s = src_index(Y, h, scale);
    if (s.i0 != ys && s.i1 != ys) continue;
    const float r = R[(((size_t)b * H + Y) * w + xs) * K + k];
    if (s.i0 == ys) a += s.l0 * r;
    if (s.i1 == ys) a += s.l1 * r;
  }
  dz[idx] = a;
}

// ---------------------------------------------------------------------------------------------------- parameter grads
// Gp [s, K, C] = dZ_s^T x_hat_s over slab s of kSlab rows; blocks of the first channel tile also write dbp [s, K].
__global__ __launch_bounds__(256) void seg_pgrad_partial_kernel(const float* __restrict__ x, const float* __restrict__ dz,
                                                                int64_t n, int C, int K, const float* __restrict__ folded,
                                                                float* __restrict__ Gp, float* __restrict__ dbp) {
  const float* mu = folded + (size_t)K * C + K;
  const float* invstd = mu + C;
  const float* mu_lo = mu + 2 * C;
  const int s = blockIdx.z;
  const int64_t r0 = (int64_t)s * kSlab, r1 = min(n, r0 + kSlab);
  head_pgrad_slab(r0, r1, s, dz, C, K, [&](int64_t row, int c) { return ((x[row * C + c] - mu[c]) - mu_lo[c]) * invstd[c]; },
                  Gp, dbp);
}

// Grid (C / 64, K): G [k, c] = sum_s Gp; dW = gamma_c G + beta_c db_k; db.
__global__ __launch_bounds__(64) void seg_pgrad_finish_kernel(const float* __restrict__ Gp, const float* __restrict__ dbp,
                                                              int S, int C, int K, const float* __restrict__ params,
                                                              int64_t off_b, int64_t off_g, int64_t off_beta,
                                                              float* __restrict__ grads, float* __restrict__ Gfin,
                                                              float* __restrict__ dbfin) {
  const int c = blockIdx.x * 64 + threadIdx.x, k = blockIdx.y;
  float G = 0.f, db = 0.f;
  for (int s = 0; s < S; ++s) {
    G += Gp[((size_t)s * K + k) * C + c];
    db += dbp[(size_t)s * K + k];
  }
  Gfin[(size_t)k * C + c] = G;
  grads[(size_t)k * C + c] = params[off_g + c] * G + params[off_beta + c] * db;
  if (c == 0) {
    grads[off_b + k] = db;
    dbfin[k] = db;
  }
}

// dgamma_c = sum_k W [k, c] G [k, c];  dbeta_c = sum_k W [k, c] db_k.
__global__ __launch_bounds__(64) void seg_pgrad_bn_kernel(const float* __restrict__ Gfin, const float* __restrict__ dbfin,
                                                          int C, int K, const float* __restrict__ params, int64_t off_g,
                                                          int64_t off_beta, float* __restrict__ grads) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  float dg = 0.f, dbeta = 0.f;
  for (int k = 0; k < K; ++k) {
    const float wkc = params[(size_t)k * C + c];
    dg += wkc * Gfin[(size_t)k * C + c];
    dbeta += wkc * dbfin[k];
  }
  grads[off_g + c] = dg;
  grads[off_beta + c] = dbeta;
}

// ---------------------------------------------------------------------------------------------------- inference
__global__ __launch_bounds__(256) void seg_slide_accum_kernel(const float* __restrict__ z, int h, int w, int K, int ch,
                                                              int cw, int y0, int x0, float* __restrict__ canvas,
                                                              float* __restrict__ count, int H, int W) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)ch * cw) return;
  const int Y = (int)(idx / cw), X = (int)(idx % cw);
  const Src sy = src_index(Y, h, (float)h / (float)ch);
  const Src sx = src_index(X, w, (float)w / (float)cw);
  const float* z00 = z + ((size_t)sy.i0 * w + sx.i0) * K;
  const float* z01 = z + ((size_t)sy.i0 * w + sx.i1) * K;
  const float* z10 = z + ((size_t)sy.i1 * w + sx.i0) * K;
  const float* z11 = z + ((size_t)sy.i1 * w + sx.i1) * K;
  const size_t plane = (size_t)H * W, o = (size_t)(y0 + Y) * W + (x0 + X);
  for (int k = 0; k < K; ++k) {
    const float v = sy.l0 * (sx.l0 * z00[k] + sx.l1 * z01[k]) + sy.l1 * (sx.l0 * z10[k] + sx.l1 * z11[k]);
    canvas[k * plane + o] += v;
  }
  count[o] += 1.f;
}

__global__ __launch_bounds__(256) void seg_finalize_kernel(const float* __restrict__ canvas, const float* __restrict__ count,
                                                           int K, int H, int W, const uint8_t* __restrict__ label,
                                                           int oh, int ow, int reduce_zero_label,
                                                           unsigned long long* __restrict__ hist,
                                                           int32_t* __restrict__ pred) {
  __shared__ unsigned int lh[3 * DVT_SEG_MAX_CLASSES];
  for (int i = threadIdx.x; i < 3 * K; i += 256) lh[i] = 0u;
  __syncthreads();
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < (int64_t)oh * ow) {
    const int Y = (int)(idx / ow), X = (int)(idx % ow);
    const Src sy = src_index(Y, H, (float)H / (float)oh);
    const Src sx = src_index(X, W, (float)W / (float)ow);
    const size_t plane = (size_t)H * W;
    const size_t o00 = (size_t)sy.i0 * W + sx.i0, o01 = (size_t)sy.i0 * W + sx.i1;
    const size_t o10 = (size_t)sy.i1 * W + sx.i0, o11 = (size_t)sy.i1 * W + sx.i1;
    const float n00 = count[o00], n01 = count[o01], n10 = count[o10], n11 = count[o11];
    float best = -INFINITY;
    int arg = 0;
    for (int k = 0; k < K; ++k) {
      const float* ck = canvas + k * plane;
      const float v = sy.l0 * (sx.l0 * (ck[o00] / n00) + sx.l1 * (ck[o01] / n01)) +
                      sy.l1 * (sx.l0 * (ck[o10] / n10) + sx.l1 * (ck[o11] / n11));
      if (v > best) {
        best = v;
        arg = k;
      }
    }
    if (pred) pred[idx] = arg;
    if (label) {
      int l = label[idx];
      if (reduce_zero_label) l = (l == 0 || l == 255) ? 255 : l - 1;
      if (l != 255) {
        atomicAdd(&lh[K + arg], 1u);
        if (l < K) {
          atomicAdd(&lh[2 * K + l], 1u);
          if (arg == l) atomicAdd(&lh[l], 1u);
        }
      }
    }
  }
  __syncthreads();
  if (label)
    for (int i = threadIdx.x; i < 3 * K; i += 256)
      if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
}

// ---------------------------------------------------------------------------------------------------- layout
void param_offsets(int C, int K, int64_t* o) {
  auto up4 = [](int64_t v) { return (v + 3) & ~(int64_t)3; };
  o[0] = 0;
  o[1] = up4((int64_t)K * C);
  o[2] = o[1] + up4(K);
  o[3] = o[2] + up4(C);
  o[4] = o[3] + up4(C);
}

struct Layout {
  size_t folded, parts, stats, z, dz, R, rowpart, Gp, dbp, Gfin, dbfin, total;
};

Layout layout(int B, int h, int w, int C, int K, int H, int W) {
  (void)W;
  const int64_t n = (int64_t)B * h * w;
  const int64_t P = (n + kStatRows - 1) / kStatRows, S = (n + kSlab - 1) / kSlab;
  Layout L;
  size_t off = 0;
  auto take = [&](size_t floats) {
    const size_t at = off;
    off += align256(floats * sizeof(float));
    return at;
  };
  L.folded = take((size_t)K * C + K + 3 * (size_t)C);
  L.parts = take((size_t)P * (3 * C + 4));
  L.stats = take(3 * (size_t)C + 4);
  L.z = take((size_t)n * K);
  L.dz = take((size_t)n * K);
  L.R = take((size_t)B * H * w * K);
  L.rowpart = take((size_t)B * H * 4);
  L.Gp = take((size_t)S * K * C);
  L.dbp = take((size_t)S * K);
  L.Gfin = take((size_t)K * C);
  L.dbfin = take((size_t)K);
  L.total = off;
  return L;
}

bool shape_ok(int C, int K) { return C > 0 && C % 64 == 0 && K >= 1 && K <= DVT_SEG_MAX_CLASSES; }

size_t loss_lds_bytes(int w, int K) { return (size_t)(w + kChunk) * K * sizeof(float); }

int launch_stats(const float* x, int64_t n, int C, float* parts, float* stats, hipStream_t s) {
  const int P = (int)((n + kStatRows - 1) / kStatRows);
  hipLaunchKernelGGL(seg_stats_kernel, dim3(P), dim3(256), 0, s, x, n, C, parts);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(seg_merge_kernel, dim3(dvt_cdiv(C, 256)), dim3(256), 0, s, parts, P, C, stats);
  DVT_CHECK_LAUNCH();
  return 0;
}

int launch_head(const float* params, const float* stats, float* running, const float* x, int64_t n, int C, int K,
                int training, float momentum, float eps, float* folded, float* z, hipStream_t s) {
  int64_t o[5];
  param_offsets(C, K, o);
  hipLaunchKernelGGL(seg_fold_kernel, dim3(K + 1), dim3(256), 0, s, params, stats, running, C, K, o[1], o[2], o[3],
                     training, momentum, eps, folded);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(seg_logits_kernel, dim3((unsigned)((n + 63) / 64), dvt_cdiv(K, 64)), dim3(256), 0, s, x, n, C, K,
                     (const float*)folded, z);
  DVT_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// ==================================================================================================== C ABI
extern "C" int dvt_seg_param_offsets(int C, int K, int64_t* out) {
  if (!out || !shape_ok(C, K)) return DVT_E_BADARG;
  param_offsets(C, K, out);
  return 0;
}

extern "C" int dvt_seg_stats_parts(int64_t n_rows) {
  if (n_rows <= 0) return DVT_E_BADARG;
  return (int)((n_rows + kStatRows - 1) / kStatRows);
}

extern "C" int64_t dvt_seg_workspace_bytes(int batch, int h, int w, int C, int K, int label_h, int label_w) {
  if (batch < 1 || h < 1 || w < 1 || label_h < 0 || label_w < 0 || !shape_ok(C, K)) return DVT_E_BADARG;
  return (int64_t)layout(batch, h, w, C, K, label_h, label_w).total;
}

extern "C" int dvt_seg_bn_stats(const float* x, int64_t n_rows, int C, float* parts, float* stats, void* stream) {
  if (!x || !parts || !stats || n_rows <= 0 || C <= 0 || C % 64) return DVT_E_BADARG;
  return launch_stats(x, n_rows, C, parts, stats, (hipStream_t)stream);
}

extern "C" int dvt_seg_bn_merge(const float* parts, int n_parts, int C, float* stats, void* stream) {
  if (!parts || !stats || n_parts < 1 || C <= 0 || C % 64) return DVT_E_BADARG;
  hipLaunchKernelGGL(seg_merge_kernel, dim3(dvt_cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, parts, n_parts, C,
                     stats);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int dvt_seg_train_step(const float* params, float* grads, float* running, const float* x,
                                  const uint8_t* labels, const float* stats, int batch, int h, int w, int C, int K,
                                  int label_h, int label_w, float momentum, float eps, void* work, int64_t work_bytes,
                                  float* out, void* stream) {
  if (!params || !grads || !running || !x || !labels || !work || !out || batch < 1 || h < 1 || w < 1 ||
      label_h < 1 || label_w < 1 || !shape_ok(C, K))
    return DVT_E_BADARG;
  if (loss_lds_bytes(w, K) > 65536 - 1024) return DVT_E_NOTIMPL;  // the static LDS of the kernel sits beside it
  const Layout L = layout(batch, h, w, C, K, label_h, label_w);
  if (work_bytes < (int64_t)L.total) return DVT_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  char* wb = (char*)work;
  auto F = [&](size_t off) { return (float*)(wb + off); };
  const int64_t n = (int64_t)batch * h * w;
  if (!stats) {
    const int rc = launch_stats(x, n, C, F(L.parts), F(L.stats), s);
    if (rc) return rc;
    stats = F(L.stats);
  }
  int rc = launch_head(params, stats, running, x, n, C, K, 1, momentum, eps, F(L.folded), F(L.z), s);
  if (rc) return rc;
  const int rows = batch * label_h;
  const float inv_total = (float)(1.0 / ((double)rows * label_w));
  hipLaunchKernelGGL(seg_loss_row_kernel, dim3(rows), dim3(256), loss_lds_bytes(w, K), s, (const float*)F(L.z), labels,
                     h, w, K, label_h, label_w, inv_total, F(L.R), F(L.rowpart));
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(seg_loss_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)F(L.rowpart), rows, inv_total, out);
  DVT_CHECK_LAUNCH();
  const int64_t nz = n * K;
  hipLaunchKernelGGL(seg_dz_kernel, dim3(dvt_cdiv(nz, 256)), dim3(256), 0, s, (const float*)F(L.R), batch, h, w, K,
                     label_h, F(L.dz));
  DVT_CHECK_LAUNCH();
  const int S = (int)((n + kSlab - 1) / kSlab);
  hipLaunchKernelGGL(seg_pgrad_partial_kernel, dim3(C / 64, dvt_cdiv(K, 64), S), dim3(256), 0, s, x,
                     (const float*)F(L.dz), n, C, K, (const float*)F(L.folded), F(L.Gp), F(L.dbp));
  DVT_CHECK_LAUNCH();
  int64_t o[5];
  param_offsets(C, K, o);
  hipLaunchKernelGGL(seg_pgrad_finish_kernel, dim3(C / 64, K), dim3(64), 0, s, (const float*)F(L.Gp),
                     (const float*)F(L.dbp), S, C, K, params, o[1], o[2], o[3], grads, F(L.Gfin), F(L.dbfin));
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(seg_pgrad_bn_kernel, dim3(C / 64), dim3(64), 0, s, (const float*)F(L.Gfin),
                     (const float*)F(L.dbfin), C, K, params, o[2], o[3], grads);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int dvt_seg_forward(const float* params, const float* running, const float* x, int64_t n_rows, int C, int K,
                               float eps, float* z, void* work, int64_t work_bytes, void* stream) {
  if (!params || !running || !x || !z || !work || n_rows < 1 || !shape_ok(C, K)) return DVT_E_BADARG;
  const size_t need = align256(((size_t)K * C + K + 3 * (size_t)C) * sizeof(float));
  if (work_bytes < (int64_t)need) return DVT_E_BADARG;
  return launch_head(params, nullptr, const_cast<float*>(running), x, n_rows, C, K, 0, 0.f, eps, (float*)work, z,
                     (hipStream_t)stream);
}

extern "C" int dvt_seg_slide_accum(const float* z, int h, int w, int K, int crop_h, int crop_w, int y0, int x0,
                                   float* canvas, float* count, int H, int W, void* stream) {
  if (!z || !canvas || !count || h < 1 || w < 1 || K < 1 || K > DVT_SEG_MAX_CLASSES || crop_h < 1 || crop_w < 1 ||
      y0 < 0 || x0 < 0 || y0 + crop_h > H || x0 + crop_w > W)
    return DVT_E_BADARG;
  hipLaunchKernelGGL(seg_slide_accum_kernel, dim3(dvt_cdiv((int64_t)crop_h * crop_w, 256)), dim3(256), 0,
                     (hipStream_t)stream, z, h, w, K, crop_h, crop_w, y0, x0, canvas, count, H, W);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int dvt_seg_finalize(const float* canvas, const float* count, int K, int H, int W, const uint8_t* label,
                                int out_h, int out_w, int reduce_zero_label, int64_t* hist, int32_t* pred, void* stream) {
  if (!canvas || !count || K < 1 || K > DVT_SEG_MAX_CLASSES || H < 1 || W < 1 || out_h < 1 || out_w < 1 ||
      (label && !hist) || (!label && !pred))
    return DVT_E_BADARG;
  hipLaunchKernelGGL(seg_finalize_kernel, dim3(dvt_cdiv((int64_t)out_h * out_w, 256)), dim3(256), 0,
                     (hipStream_t)stream, canvas, count, K, H, W, label, out_h, out_w, reduce_zero_label,
                     (unsigned long long*)hist, pred);
  DVT_CHECK_LAUNCH();
  return 0;
}
