// Linear-probe depth head and evaluation (include/dvt_depth.h): the reference's depth BNHead (no norm layer) with
// conv_depth, SigLoss + GradientLoss, gradient clipping and the NYU metrics, in exact fp32 with fixed-order reductions.
//
// The 1 x 1 convolution commutes with the bilinear upsample, so the logits live at TOKEN resolution and the [B, 2C, up h,
// up w] tensor of the reference is never made.  Training step, per batch (no host synchronisation, ten launches, eleven
// for a batch of three or more, which adds depth_vgrad_kernel):
//   depth_cls_kernel            zc [B, K] = cls W[:, C:]^T + b
//   depth_logits_kernel         Z [B h w, K] = X W[:, :C]^T + zc, a 64 x 64 fp32 tile
//   depth_pixel_kernel          one wave per pixel of the up h x up w map: the K interpolated logits, p = relu + 0.1,
//                               sum p, depth = sum p bin / sum p; keeps depth, sum p and the relu mask (K bits)
//   depth_loss_stats_kernel     the resize to the ground truth, g = log(pred + eps) - log(gt + eps), and one
//                               (count, mean, M2) record per block of 1024 pixels
//   depth_vgrad_kernel          (batch >= 3) the gradient loss's |g_j - g_{j+2}| sums per block and sub-sampling
//   depth_loss_finish_kernel    Chan's merge of the records in fp64, both losses, the coefficients of dL/dg
//   depth_adj_x_kernel /
//   depth_adj_y_kernel          dL/dpred per pixel and the adjoint of the resize as a gather, along x and then y
//   depth_dz_kernel             one workgroup per token: the adjoint of the upsample, with
//                               d depth / d z_k = relu'(z_k) (bin_k - depth) / sum p, into dZ [B h w, K]
//   depth_pgrad_partial_kernel  G_s = dZ_s^T X_s and the column sums of dZ_s over slabs of 256 rows of one image
//   depth_pgrad_finish_kernel   dW[:, :C] = sum_s G_s, dW[:, C:] = sum_b (sum of dZ_b) (x) cls_b, db
//
// The bilinear source index and the two 64 x 64 tiles (logits, parameter-gradient slab) are dvt_head_dev.h's, shared with
// the segmentation head.
#include "dvt_head_dev.h"
#include "../../include/dvt_depth.h"

#include <assert.h>
#include <math.h>

namespace {

constexpr int kSlab = 256;      // rows per parameter-gradient slab
constexpr int kLossPix = 1024;  // pixels per loss record
constexpr int kClipBlock = 4096;
constexpr float kEps = 1e-3f;   // SigLoss / GradientLoss eps
constexpr int kMaxCand = (2 * DVT_DEPTH_MAX_UP + 4) * (2 * DVT_DEPTH_MAX_UP + 4);  // cand_range: at most 2 up + 4 per axis

// Destination indices that can read source index `src` (a superset; the caller tests each with src_index).
__device__ __forceinline__ void cand_range(int src, float scale, int out, int* lo, int* hi) {
  const float inv = 1.f / scale;
  int a = (int)floorf(((float)src - 0.5f) * inv - 0.5f) - 1;
  int b = (int)ceilf(((float)src + 1.5f) * inv - 0.5f) + 1;
  *lo = a < 0 ? 0 : a;
  *hi = b > out - 1 ? out - 1 : b;
}

// Weight with which destination `dst` reads source `src`.
__device__ __forceinline__ float src_weight(int dst, int in, float scale, int src) {
  const Src r = src_index(dst, in, scale);
  return (r.i0 == src ? r.l0 : 0.f) + (r.i1 == src ? r.l1 : 0.f);
}

__device__ __forceinline__ float bilinear(const float* __restrict__ img, int w, const Src& sy, const Src& sx) {
  const float* r0 = img + (size_t)sy.i0 * w;
  const float* r1 = img + (size_t)sy.i1 * w;
  return sy.l0 * (sx.l0 * r0[sx.i0] + sx.l1 * r0[sx.i1]) + sy.l1 * (sx.l0 * r1[sx.i0] + sx.l1 * r1[sx.i1]);
}

// Fixed-order tree sum over the 256 threads of a block; every thread gets the result.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// ---------------------------------------------------------------------------------------------------- forward
// zc [b, k] = bias_k + sum_c cls [b, c] W [k, C + c]; one wave per (b, k).
__global__ __launch_bounds__(256) void depth_cls_kernel(const float* __restrict__ params, const float* __restrict__ cls,
                                                        int C, int K, int64_t off_b, float* __restrict__ zc) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y, lane = threadIdx.x & 63;
  if (k >= K) return;
  const float* wr = params + (size_t)k * 2 * C + C;
  const float* cr = cls + (size_t)b * C;
  float acc = 0.f;
  for (int c = lane; c < C; c += 64) acc = fmaf(cr[c], wr[c], acc);
  acc = wave_sum(acc);
  if (lane == 0) zc[(size_t)b * K + k] = acc + params[off_b + k];
}

// Z [n, K] = X W[:, :C]^T + zc [image of the row].  Tile 64 rows x 64 bins, 32 channels per stage; thread (ty, tx) owns 4 x 4.
__global__ __launch_bounds__(256) void depth_logits_kernel(const float* __restrict__ x, int64_t n, int hw, int C, int K,
                                                           const float* __restrict__ params, const float* __restrict__ zc,
                                                           float* __restrict__ z) {
  const int64_t n0 = (int64_t)blockIdx.x * 64;
  const int k0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc[4][4] = {};
  head_logits_tile(n0, n, k0, K, C, [&](int64_t row, int c) { return x[row * C + c]; },
                   [&](int kk, int c) { return params[(size_t)kk * 2 * C + c]; }, acc);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = n0 + ty * 4 + i;
    if (row >= n) continue;
    const float* zr = zc + (size_t)(row / hw) * K;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kk = k0 + tx * 4 + j;
      if (kk < K) z[row * K + kk] = acc[i][j] + zr[kk];
    }
  }
}

// One wave per pixel of the [B, uh, uw] map.  mask (may be NULL): 4 words of 64 bits per pixel, bit (k & 63) of word
// (k >> 6) = z_k > 0.
// The relu's side decides a whole term of the gradient, and fp32 rounding of a logit next to 0 can take the other side
// than the exact value (measured: about one logit in 10^7, which moves dW by up to 7e-4 of its norm).  So the SIDE of a
// logit below 1e-5 of the pixel's mean |z| is decided in fp64 from the features and weights; the forward value stays the
// fp32 one.  Cost: 5 C / 64 fp64 multiply-adds per lane and such logit, so the step time grows with their number.
__global__ __launch_bounds__(256) void depth_pixel_kernel(const float* __restrict__ z, const float* __restrict__ bins,
                                                          const float* __restrict__ x, const float* __restrict__ cls,
                                                          const float* __restrict__ params, int C, int B, int h, int w,
                                                          int K, int uh, int uw, float* __restrict__ depth,
                                                          float* __restrict__ psum, unsigned long long* __restrict__ mask) {
  const int64_t pix = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (pix >= (int64_t)B * uh * uw) return;
  const int b = (int)(pix / ((int64_t)uh * uw));
  const int rem = (int)(pix - (int64_t)b * uh * uw);
  const int y = rem / uw, xx = rem - y * uw;
  const Src sy = src_index(y, h, (float)h / (float)uh), sx = src_index(xx, w, (float)w / (float)uw);
  const size_t t00 = ((size_t)b * h + sy.i0) * w + sx.i0, t01 = ((size_t)b * h + sy.i0) * w + sx.i1;
  const size_t t10 = ((size_t)b * h + sy.i1) * w + sx.i0, t11 = ((size_t)b * h + sy.i1) * w + sx.i1;
  float v[4];
  float asum = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = lane + 64 * i;
    v[i] = 0.f;
    if (k < K) {
      v[i] = sy.l0 * (sx.l0 * z[t00 * K + k] + sx.l1 * z[t01 * K + k]) +
             sy.l1 * (sx.l0 * z[t10 * K + k] + sx.l1 * z[t11 * K + k]);
      asum += fabsf(v[i]);
    }
  }
  const float thr = 1e-5f * wave_sum(asum) / (float)K;
  float S = 0.f, E = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = lane + 64 * i;
    bool pos = false;
    if (k < K) {
      pos = v[i] > 0.f;
    }
    // the exact side of the relu for the logits next to 0: the whole wave takes them one by one, lanes over the channels
    unsigned long long need = __ballot(k < K && fabsf(v[i]) < thr);
    while (need) {
      const int src = __ffsll((long long)need) - 1;
      need &= need - 1;
      const float* wr = params + (size_t)(src + 64 * i) * 2 * C;
      double zc = 0.0, a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
      for (int c = lane; c < C; c += 64) {
        const double wc = (double)wr[c];
        zc += (double)cls[(size_t)b * C + c] * (double)wr[C + c];
        a00 += (double)x[t00 * C + c] * wc;
        a01 += (double)x[t01 * C + c] * wc;
        a10 += (double)x[t10 * C + c] * wc;
        a11 += (double)x[t11 * C + c] * wc;
      }
      const double e = (double)sy.l0 * ((double)sx.l0 * wave_sum_f64(a00) + (double)sx.l1 * wave_sum_f64(a01)) +
                       (double)sy.l1 * ((double)sx.l0 * wave_sum_f64(a10) + (double)sx.l1 * wave_sum_f64(a11)) +
                       wave_sum_f64(zc) + (double)params[(size_t)K * 2 * C + src + 64 * i];
      if (lane == src) pos = e > 0.0;
    }
    if (k < K) {
      const float p = (pos ? v[i] : 0.f) + 0.1f;
      S += p;
      E = fmaf(p, bins[k], E);
    }
    const unsigned long long m = __ballot(pos);
    if (mask && lane == 0) mask[pix * 4 + i] = m;
  }
  S = wave_sum(S);
  E = wave_sum(E);
  if (lane == 0) {
    depth[pix] = E / S;
    if (psum) psum[pix] = S;
  }
}

// ---------------------------------------------------------------------------------------------------- loss
// Grid (P, B).  g [B, H, W] (0 where invalid), rp = 1 / (pred + eps), rec [B, P, 4] = count, mean, M2, 0.
__global__ __launch_bounds__(256) void depth_loss_stats_kernel(const float* __restrict__ depth, const float* __restrict__ gt,
                                                               int uh, int uw, int H, int W, float* __restrict__ g,
                                                               float* __restrict__ rp, float* __restrict__ rec) {
  __shared__ float red[256];
  const int b = blockIdx.y, P = gridDim.x;
  const int HW = H * W;
  const float* db = depth + (size_t)b * uh * uw;
  const float sy_scale = (float)uh / (float)H, sx_scale = (float)uw / (float)W;
  float gv[4];
  bool ok[4];
  float cnt = 0.f, sum = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int idx = blockIdx.x * kLossPix + j * 256 + threadIdx.x;
    gv[j] = 0.f;
    ok[j] = false;
    if (idx < HW) {
      const int y = idx / W, xx = idx - y * W;
      const float pr = bilinear(db, uw, src_index(y, uh, sy_scale), src_index(xx, uw, sx_scale)) + kEps;
      const float t = gt[(size_t)b * HW + idx];
      ok[j] = t > 0.f;
      if (ok[j]) gv[j] = logf(pr) - logf(t + kEps);
      g[(size_t)b * HW + idx] = gv[j];
      rp[(size_t)b * HW + idx] = 1.f / pr;
      if (ok[j]) {
        cnt += 1.f;
        sum += gv[j];
      }
    }
  }
  cnt = block_sum(cnt, red);
  sum = block_sum(sum, red);
  const float mean = cnt > 0.f ? sum / cnt : 0.f;
  float m2 = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (ok[j]) m2 = fmaf(gv[j] - mean, gv[j] - mean, m2);
  m2 = block_sum(m2, red);
  if (threadIdx.x == 0) {
    float* r = rec + ((size_t)b * P + blockIdx.x) * 4;
    r[0] = cnt;
    r[1] = mean;
    r[2] = m2;
    r[3] = 0.f;
  }
}

// The sub-samplings of the gradient loss: strides 1, 2, 4, 6 over the batch axis.
__device__ __forceinline__ int grad_stride(int si) { return si == 0 ? 1 : 2 * si; }

// Grid (P, B): vparts [B, P, 4] = per sub-sampling, sum over the block's pixels of |g_b - g_partner| where both are valid;
// partner = the image two places on in the sub-sampled batch (0 where there is none).
__global__ __launch_bounds__(256) void depth_vgrad_kernel(const float* __restrict__ g, const float* __restrict__ gt, int B,
                                                          int HW, float* __restrict__ vparts) {
  __shared__ float red[256];
  const int b = blockIdx.y, P = gridDim.x;
  for (int si = 0; si < 4; ++si) {
    const int s = grad_stride(si);
    float acc = 0.f;
    if (b % s == 0) {
      const int j = b / s, Bs = (B + s - 1) / s;
      if (j + 2 < Bs) {
        const int p = s * (j + 2);
        for (int q = 0; q < 4; ++q) {
          const int idx = blockIdx.x * kLossPix + q * 256 + threadIdx.x;
          if (idx < HW && gt[(size_t)b * HW + idx] > 0.f && gt[(size_t)p * HW + idx] > 0.f)
            acc += fabsf(g[(size_t)b * HW + idx] - g[(size_t)p * HW + idx]);
        }
      }
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) vparts[((size_t)b * P + blockIdx.x) * 4 + si] = acc;
  }
}

struct Rec {
  double n, mean, m2;
};

__device__ __forceinline__ Rec merge(const Rec& a, const Rec& b) {  // Chan's rule
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  Rec r;
  r.n = a.n + b.n;
  const double d = b.mean - a.mean;
  r.mean = a.mean + d * (b.n / r.n);
  r.m2 = a.m2 + b.m2 + d * d * (a.n * b.n / r.n);
  return r;
}

// One block.  coef [8] = a, c, mean, w_0 .. w_3, 0:  dL/dg_i = a (g_i - mean) + c  (+ the gradient loss's terms with weights
// w_si = grad_weight / N_si).  out [2] = loss_depth, grad_weight * gradient loss.
__global__ __launch_bounds__(256) void depth_loss_finish_kernel(const float* __restrict__ rec,
                                                                const float* __restrict__ vparts, int B, int P, int warm_up,
                                                                float grad_weight, float* __restrict__ coef,
                                                                float* __restrict__ out) {
  __shared__ Rec recs[256];
  __shared__ double cnt_img[DVT_DEPTH_MAX_BATCH];
  __shared__ double vsum[4];
  __shared__ double vred[256];
  const int R = B * P;
  const int chunk = (R + 255) / 256;
  Rec a = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x * chunk; i < min(R, ((int)threadIdx.x + 1) * chunk); ++i) {
    const Rec r = {(double)rec[(size_t)i * 4], (double)rec[(size_t)i * 4 + 1], (double)rec[(size_t)i * 4 + 2]};
    a = merge(a, r);
  }
  recs[threadIdx.x] = a;
  if ((int)threadIdx.x < B) {
    double c = 0.0;
    for (int i = 0; i < P; ++i) c += (double)rec[((size_t)threadIdx.x * P + i) * 4];
    cnt_img[threadIdx.x] = c;
  }
  for (int si = 0; si < 4; ++si) {  // the same chunks and tree as the records
    double v = 0.0;
    if (vparts)
      for (int i = threadIdx.x * chunk; i < min(R, ((int)threadIdx.x + 1) * chunk); ++i) v += (double)vparts[(size_t)i * 4 + si];
    v = block_sum(v, vred);
    if (threadIdx.x == 0) vsum[si] = v;
  }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) recs[threadIdx.x] = merge(recs[threadIdx.x], recs[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const Rec t = recs[0];
  const double N = t.n, m = t.mean;
  double loss, ca = 0.0, cc = 0.0;
  bool ok = true;
  if (N < 1.0 || (!warm_up && N < 2.0)) {
    loss = nan("");
    ok = false;
  } else if (warm_up) {
    loss = sqrt(0.15 * m * m);
    if (loss > 0.0) cc = 0.15 * m / (N * loss);
  } else {
    loss = sqrt(t.m2 / (N - 1.0) + 0.15 * m * m);
    if (loss > 0.0) {
      ca = 1.0 / ((N - 1.0) * loss);
      cc = 0.15 * m / (N * loss);
    }
  }
  double lgrad = 0.0;
  float wgt[4] = {0.f, 0.f, 0.f, 0.f};
  if (vparts) {
    for (int si = 0; si < 4; ++si) {
      const int s = grad_stride(si);
      double Ns = 0.0;
      for (int b = 0; b < B; b += s) Ns += cnt_img[b];
      if (Ns > 0.0) {
        lgrad += vsum[si] / Ns;
        if (ok) wgt[si] = (float)((double)grad_weight / Ns);
      }
    }
  }
  coef[0] = (float)ca;
  coef[1] = (float)cc;
  coef[2] = (float)m;
  for (int si = 0; si < 4; ++si) coef[3 + si] = wgt[si];
  coef[7] = 0.f;
  out[0] = (float)loss;
  out[1] = (float)((double)grad_weight * lgrad);
}

// dL/dpred at pixel idx of image b.
__device__ __forceinline__ float dpred_at(const float* __restrict__ g, const float* __restrict__ rp,
                                          const float* __restrict__ gt, const float* __restrict__ coef, int B, int HW, int b,
                                          int idx) {
  const size_t at = (size_t)b * HW + idx;
  if (!(gt[at] > 0.f)) return 0.f;
  const float gv = g[at];
  float d = fmaf(coef[0], gv - coef[2], coef[1]);
  if (B >= 3) {
    for (int si = 0; si < 4; ++si) {
      const int s = grad_stride(si);
      const float wv = coef[3 + si];
      if (b % s != 0 || wv == 0.f) continue;
      const int j = b / s, Bs = (B + s - 1) / s;
      if (j + 2 < Bs) {
        const size_t pa = (size_t)(s * (j + 2)) * HW + idx;
        if (gt[pa] > 0.f) {
          const float df = gv - g[pa];
          d += df > 0.f ? wv : df < 0.f ? -wv : 0.f;
        }
      }
      if (j - 2 >= 0) {
        const size_t pa = (size_t)(s * (j - 2)) * HW + idx;
        if (gt[pa] > 0.f) {
          const float df = gv - g[pa];
          d += df > 0.f ? wv : df < 0.f ? -wv : 0.f;
        }
      }
    }
  }
  return d * rp[at];
}

// R [B, H, uw]: the adjoint of the resize along x, a gather over the destination columns that read column sx.
__global__ __launch_bounds__(256) void depth_adj_x_kernel(const float* __restrict__ g, const float* __restrict__ rp,
                                                          const float* __restrict__ gt, const float* __restrict__ coef,
                                                          int B, int H, int W, int uw, float* __restrict__ Rx) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)B * H * uw) return;
  const int sx = (int)(t % uw);
  const int64_t by = t / uw;
  const int y = (int)(by % H), b = (int)(by / H);
  const float scale = (float)uw / (float)W;
  int lo, hi;
  cand_range(sx, scale, W, &lo, &hi);
  float acc = 0.f;
  for (int xx = lo; xx <= hi; ++xx) {
    const float wt = src_weight(xx, uw, scale, sx);
    if (wt != 0.f) acc = fmaf(wt, dpred_at(g, rp, gt, coef, B, H * W, b, y * W + xx), acc);
  }
  Rx[t] = acc;
}

// D [B, uh, uw] = dL/d depth: the adjoint along y.
__global__ __launch_bounds__(256) void depth_adj_y_kernel(const float* __restrict__ Rx, int B, int H, int uh, int uw,
                                                          float* __restrict__ D) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)B * uh * uw) return;
  const int sx = (int)(t % uw);
  const int64_t by = t / uw;
  const int sy = (int)(by % uh), b = (int)(by / uh);
  const float scale = (float)uh / (float)H;
  int lo, hi;
  cand_range(sy, scale, H, &lo, &hi);
  float acc = 0.f;
  for (int y = lo; y <= hi; ++y) {
    const float wt = src_weight(y, uh, scale, sy);
    if (wt != 0.f) acc = fmaf(wt, Rx[((size_t)b * H + y) * uw + sx], acc);
  }
  D[t] = acc;
}

// One workgroup per token, thread = bin: dZ [token, k] = sum over the map pixels that read the token of
//   wy wx D / sum p * relu'(z_k) (bin_k - depth).
__global__ __launch_bounds__(256) void depth_dz_kernel(const float* __restrict__ D, const float* __restrict__ depth,
                                                       const float* __restrict__ psum,
                                                       const unsigned long long* __restrict__ mask,
                                                       const float* __restrict__ bins, int h, int w, int K, int uh, int uw,
                                                       float* __restrict__ dz) {
  __shared__ float q[kMaxCand];
  __shared__ float dep[kMaxCand];
  __shared__ int64_t pixs[kMaxCand];
  const int token = blockIdx.x;
  const int b = token / (h * w), rem = token - b * h * w;
  const int ty = rem / w, tx = rem - ty * w;
  const float sys = (float)h / (float)uh, sxs = (float)w / (float)uw;
  int ylo, yhi, xlo, xhi;
  cand_range(ty, sys, uh, &ylo, &yhi);
  cand_range(tx, sxs, uw, &xlo, &xhi);
  const int ny = yhi - ylo + 1, nx = xhi - xlo + 1;
  // cand_range returns at most 2 up + 4 indices per axis (up <= DVT_DEPTH_MAX_UP is checked by shape_ok), so ny nx <= kMaxCand
  const int nc = ny * nx;
  assert(nc <= kMaxCand);
  for (int e = threadIdx.x; e < nc; e += 256) {
    const int y = ylo + e / nx, xx = xlo + e % nx;
    const float wt = src_weight(y, h, sys, ty) * src_weight(xx, w, sxs, tx);
    const int64_t pix = ((int64_t)b * uh + y) * uw + xx;
    pixs[e] = pix;
    q[e] = wt != 0.f ? wt * D[pix] / psum[pix] : 0.f;
    dep[e] = depth[pix];
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k >= K) return;
  const float bin = bins[k];
  float acc = 0.f;
  for (int e = 0; e < nc; ++e) {
    const float qe = q[e];
    if (qe == 0.f) continue;
    if ((mask[pixs[e] * 4 + (k >> 6)] >> (k & 63)) & 1ull) acc = fmaf(qe, bin - dep[e], acc);
  }
  dz[(size_t)token * K + k] = acc;
}

// ---------------------------------------------------------------------------------------------------- parameter grads
// Grid (C / 64, ceil(K / 64), B * Sb): slab s of image b covers rows [s kSlab, ...) of that image.  Gp [b Sb + s, K, C] =
// dZ^T X over the slab; blocks of the first channel tile also write dbp [b Sb + s, K], the slab's column sums of dZ.
__global__ __launch_bounds__(256) void depth_pgrad_partial_kernel(const float* __restrict__ x, const float* __restrict__ dz,
                                                                  int hw, int Sb, int C, int K, float* __restrict__ Gp,
                                                                  float* __restrict__ dbp) {
  const int slab = blockIdx.z;
  const int b = slab / Sb, s = slab - b * Sb;
  const int64_t base = (int64_t)b * hw;
  const int64_t r0 = base + (int64_t)s * kSlab, r1 = min(base + hw, r0 + kSlab);
  head_pgrad_slab(r0, r1, slab, dz, C, K, [&](int64_t row, int c) { return x[row * C + c]; }, Gp, dbp);
}

// Grid (2 C / 64, K).
__global__ __launch_bounds__(64) void depth_pgrad_finish_kernel(const float* __restrict__ Gp, const float* __restrict__ dbp,
                                                                const float* __restrict__ cls, int B, int Sb, int C, int K,
                                                                int64_t off_b, float* __restrict__ grads) {
  const int c = blockIdx.x * 64 + threadIdx.x, k = blockIdx.y;
  if (c < C) {
    float G = 0.f;
    for (int s = 0; s < B * Sb; ++s) G += Gp[((size_t)s * K + k) * C + c];
    grads[(size_t)k * 2 * C + c] = G;
  } else {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) {
      float dzs = 0.f;
      for (int s = 0; s < Sb; ++s) dzs += dbp[(size_t)(b * Sb + s) * K + k];
      acc = fmaf(dzs, cls[(size_t)b * C + (c - C)], acc);
    }
    grads[(size_t)k * 2 * C + c] = acc;
  }
  if (c == 0) {
    float db = 0.f;
    for (int b = 0; b < B; ++b) {
      float dzs = 0.f;
      for (int s = 0; s < Sb; ++s) dzs += dbp[(size_t)(b * Sb + s) * K + k];
      db += dzs;
    }
    grads[off_b + k] = db;
  }
}

// ---------------------------------------------------------------------------------------------------- clipping
__global__ __launch_bounds__(256) void depth_sumsq_kernel(const float* __restrict__ gr, int64_t n, float* __restrict__ parts) {
  __shared__ float red[256];
  float acc = 0.f;
  const int64_t base = (int64_t)blockIdx.x * kClipBlock;
  for (int j = 0; j < kClipBlock / 256; ++j) {
    const int64_t i = base + j * 256 + threadIdx.x;
    if (i < n) acc = fmaf(gr[i], gr[i], acc);
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) parts[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void depth_clip_finish_kernel(const float* __restrict__ parts, int n_parts, float max_norm,
                                                                float* __restrict__ out) {
  __shared__ double red[256];
  double acc = 0.0;
  const int chunk = (n_parts + 255) / 256;
  for (int i = threadIdx.x * chunk; i < min(n_parts, ((int)threadIdx.x + 1) * chunk); ++i) acc += (double)parts[i];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(acc);
    const float f = max_norm / (norm + 1e-6f);
    out[0] = norm;
    out[1] = f < 1.f ? f : 1.f;  // a NaN norm gives NaN, as torch's clamp does
    if (f != f) out[1] = f;
  }
}

__global__ __launch_bounds__(256) void depth_scale_kernel(float* __restrict__ gr, int64_t n, const float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) gr[i] *= out[1];
}

// ---------------------------------------------------------------------------------------------------- evaluation
constexpr int kEvalSums = 10;

// parts [P, 10] (fp64): count, a1, a2, a3, sum |gt - pred| / gt, sum (gt - pred)^2, sum |log10 gt - log10 pred|,
// sum (log gt - log pred)^2, sum (log pred - log gt), sum (gt - pred)^2 / gt.
__global__ __launch_bounds__(256) void depth_eval_kernel(const float* __restrict__ d0, const float* __restrict__ d1, int uh,
                                                         int uw, const float* __restrict__ gt, int oh, int ow, float dmin,
                                                         float dmax, int cy0, int cy1, int cx0, int cx1,
                                                         float* __restrict__ pred, double* __restrict__ parts) {
  __shared__ double red[256];
  const float sys = (float)uh / (float)oh, sxs = (float)uw / (float)ow;
  double acc[kEvalSums] = {};
  for (int j = 0; j < 4; ++j) {
    const int idx = blockIdx.x * kLossPix + j * 256 + threadIdx.x;
    if (idx >= oh * ow) continue;
    const int y = idx / ow, xx = idx - y * ow;
    auto sample = [&](const float* d, int xs) {
      const Src sy = src_index(y, uh, sys), sx = src_index(xs, uw, sxs);
      auto cl = [&](int yy, int xq) { return fminf(fmaxf(d[(size_t)yy * uw + xq], dmin), dmax); };
      return sy.l0 * (sx.l0 * cl(sy.i0, sx.i0) + sx.l1 * cl(sy.i0, sx.i1)) +
             sy.l1 * (sx.l0 * cl(sy.i1, sx.i0) + sx.l1 * cl(sy.i1, sx.i1));
    };
    float p = sample(d0, xx);
    if (d1) p = (p + sample(d1, ow - 1 - xx)) / 2.f;
    if (pred) pred[idx] = p;
    const float t = gt[idx];
    if (!(t > dmin && t < dmax) || y < cy0 || y >= cy1 || xx < cx0 || xx >= cx1) continue;
    const double G = (double)t, Pd = (double)p;
    const double th = fmax(G / Pd, Pd / G);
    const double df = G - Pd, lg = log(G) - log(Pd);
    acc[0] += 1.0;
    acc[1] += th < 1.25 ? 1.0 : 0.0;
    acc[2] += th < 1.25 * 1.25 ? 1.0 : 0.0;
    acc[3] += th < 1.25 * 1.25 * 1.25 ? 1.0 : 0.0;
    acc[4] += fabs(df) / G;
    acc[5] += df * df;
    acc[6] += fabs(log10(G) - log10(Pd));
    acc[7] += lg * lg;
    acc[8] += -lg;
    acc[9] += df * df / G;
  }
  for (int i = 0; i < kEvalSums; ++i) {
    const double v = block_sum(acc[i], red);
    if (threadIdx.x == 0) parts[(size_t)blockIdx.x * kEvalSums + i] = v;
  }
}

__global__ __launch_bounds__(64) void depth_eval_finish_kernel(const double* __restrict__ parts, int P, double* __restrict__ row) {
  __shared__ double sums[kEvalSums];
  if (threadIdx.x < kEvalSums) {
    double v = 0.0;
    for (int i = 0; i < P; ++i) v += parts[(size_t)i * kEvalSums + threadIdx.x];
    sums[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double n = sums[0];
  if (n < 1.0) {
    for (int i = 0; i < 9; ++i) row[i] = nan("");
    return;
  }
  row[0] = sums[1] / n;
  row[1] = sums[2] / n;
  row[2] = sums[3] / n;
  row[3] = sums[4] / n;
  row[4] = sqrt(sums[5] / n);
  row[5] = sums[6] / n;
  row[6] = sqrt(sums[7] / n);
  const double me = sums[8] / n;
  const double sil = sqrt(sums[7] / n - me * me) * 100.0;
  row[7] = sil != sil ? 0.0 : sil;
  row[8] = sums[9] / n;
}

// ---------------------------------------------------------------------------------------------------- layout
bool shape_ok(int B, int h, int w, int C, int K, int up) {
  return B >= 1 && B <= DVT_DEPTH_MAX_BATCH && h >= 1 && w >= 1 && C > 0 && C % 64 == 0 && K >= 4 && K % 4 == 0 &&
         K <= DVT_DEPTH_MAX_BINS && up >= 1 && up <= DVT_DEPTH_MAX_UP && (int64_t)B * h * w * up * up < (1LL << 30);
}

struct Layout {
  size_t zc, z, depth, psum, mask, g, rp, rec, vparts, coef, Rx, D, dz, Gp, dbp, total;
};

Layout layout(int B, int h, int w, int C, int K, int up, int H, int W) {
  const int64_t n = (int64_t)B * h * w, npix = n * up * up;
  const int64_t HW = (int64_t)H * W, P = (HW + kLossPix - 1) / kLossPix;
  const int64_t Sb = ((int64_t)h * w + kSlab - 1) / kSlab;
  Layout L;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t at = off;
    off += align256(bytes);
    return at;
  };
  L.zc = take((size_t)B * K * 4);
  L.z = take((size_t)n * K * 4);
  L.depth = take((size_t)npix * 4);
  L.psum = take((size_t)npix * 4);
  L.mask = take((size_t)npix * 4 * 8);
  L.g = take((size_t)B * HW * 4);
  L.rp = take((size_t)B * HW * 4);
  L.rec = take((size_t)B * P * 4 * 4);
  L.vparts = take((size_t)B * P * 4 * 4);
  L.coef = take(8 * 4);
  L.Rx = take((size_t)B * H * w * up * 4);
  L.D = take((size_t)npix * 4);
  L.dz = HW ? take((size_t)n * K * 4) : off;
  L.Gp = HW ? take((size_t)B * Sb * K * C * 4) : off;
  L.dbp = HW ? take((size_t)B * Sb * K * 4) : off;
  L.total = off;
  return L;
}

int launch_forward(const float* params, const float* bins, const float* x, const float* cls, int B, int h, int w, int C,
                   int K, int up, float* zc, float* z, float* depth, float* psum, unsigned long long* mask, hipStream_t s) {
  const int64_t n = (int64_t)B * h * w;
  hipLaunchKernelGGL(depth_cls_kernel, dim3(dvt_cdiv(K, 4), B), dim3(256), 0, s, params, cls, C, K, (int64_t)K * 2 * C, zc);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(depth_logits_kernel, dim3((unsigned)((n + 63) / 64), dvt_cdiv(K, 64)), dim3(256), 0, s, x, n, h * w, C,
                     K, params, (const float*)zc, z);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(depth_pixel_kernel, dim3(dvt_cdiv(n * up * up, 4)), dim3(256), 0, s, (const float*)z, bins, x, cls,
                     params, C, B, h, w, K, up * h, up * w, depth, psum, mask);
  DVT_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// ==================================================================================================== C ABI
extern "C" int dvt_depth_param_offsets(int C, int K, int64_t* out) {
  if (!out || C <= 0 || C % 64 || K < 4 || K % 4 || K > DVT_DEPTH_MAX_BINS) return DVT_E_BADARG;
  out[0] = 0;
  out[1] = (int64_t)K * 2 * C;
  out[2] = out[1] + K;
  return 0;
}

extern "C" int64_t dvt_depth_workspace_bytes(int batch, int h, int w, int C, int K, int up, int gt_h, int gt_w) {
  if (!shape_ok(batch, h, w, C, K, up) || gt_h < 0 || gt_w < 0 || (int64_t)batch * gt_h * gt_w >= (1LL << 30)) return -1;
  return (int64_t)layout(batch, h, w, C, K, up, gt_h, gt_w).total;
}

extern "C" int dvt_depth_forward(const float* params, const float* bins, const float* x, const float* cls, int batch, int h,
                                 int w, int C, int K, int up, float* depth, void* work, int64_t work_bytes, void* stream) {
  if (!params || !bins || !x || !cls || !depth || !work || !shape_ok(batch, h, w, C, K, up)) return DVT_E_BADARG;
  const Layout L = layout(batch, h, w, C, K, up, 0, 0);
  if (work_bytes < (int64_t)L.total) return DVT_E_BADARG;
  char* wb = (char*)work;
  return launch_forward(params, bins, x, cls, batch, h, w, C, K, up, (float*)(wb + L.zc), (float*)(wb + L.z), depth, nullptr,
                        nullptr, (hipStream_t)stream);
}

extern "C" int dvt_depth_train_step(const float* params, float* grads, const float* bins, const float* x, const float* cls,
                                    const float* gt, int batch, int h, int w, int C, int K, int up, int gt_h, int gt_w,
                                    int warm_up, float grad_weight, void* work, int64_t work_bytes, float* out,
                                    void* stream) {
  if (!params || !grads || !bins || !x || !cls || !gt || !work || !out || !shape_ok(batch, h, w, C, K, up) || gt_h < 1 ||
      gt_w < 1 || (int64_t)batch * gt_h * gt_w >= (1LL << 30))
    return DVT_E_BADARG;
  const Layout L = layout(batch, h, w, C, K, up, gt_h, gt_w);
  if (work_bytes < (int64_t)L.total) return DVT_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  char* wb = (char*)work;
  auto F = [&](size_t off) { return (float*)(wb + off); };
  unsigned long long* mask = (unsigned long long*)(wb + L.mask);
  const int uh = up * h, uw = up * w, HW = gt_h * gt_w;
  const int64_t n = (int64_t)batch * h * w, npix = n * up * up;
  int rc = launch_forward(params, bins, x, cls, batch, h, w, C, K, up, F(L.zc), F(L.z), F(L.depth), F(L.psum), mask, s);
  if (rc) return rc;
  const int P = (HW + kLossPix - 1) / kLossPix;
  hipLaunchKernelGGL(depth_loss_stats_kernel, dim3(P, batch), dim3(256), 0, s, (const float*)F(L.depth), gt, uh, uw, gt_h,
                     gt_w, F(L.g), F(L.rp), F(L.rec));
  DVT_CHECK_LAUNCH();
  const float* vparts = nullptr;
  if (batch >= 3) {
    hipLaunchKernelGGL(depth_vgrad_kernel, dim3(P, batch), dim3(256), 0, s, (const float*)F(L.g), gt, batch, HW,
                       F(L.vparts));
    DVT_CHECK_LAUNCH();
    vparts = F(L.vparts);
  }
  hipLaunchKernelGGL(depth_loss_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)F(L.rec), vparts, batch, P, warm_up,
                     grad_weight, F(L.coef), out);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(depth_adj_x_kernel, dim3(dvt_cdiv((int64_t)batch * gt_h * uw, 256)), dim3(256), 0, s,
                     (const float*)F(L.g), (const float*)F(L.rp), gt, (const float*)F(L.coef), batch, gt_h, gt_w, uw,
                     F(L.Rx));
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(depth_adj_y_kernel, dim3(dvt_cdiv(npix, 256)), dim3(256), 0, s, (const float*)F(L.Rx), batch, gt_h, uh,
                     uw, F(L.D));
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(depth_dz_kernel, dim3((unsigned)n), dim3(256), 0, s, (const float*)F(L.D), (const float*)F(L.depth),
                     (const float*)F(L.psum), (const unsigned long long*)mask, bins, h, w, K, uh, uw, F(L.dz));
  DVT_CHECK_LAUNCH();
  const int Sb = (h * w + kSlab - 1) / kSlab;
  hipLaunchKernelGGL(depth_pgrad_partial_kernel, dim3(C / 64, dvt_cdiv(K, 64), batch * Sb), dim3(256), 0, s, x,
                     (const float*)F(L.dz), h * w, Sb, C, K, F(L.Gp), F(L.dbp));
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(depth_pgrad_finish_kernel, dim3(2 * C / 64, K), dim3(64), 0, s, (const float*)F(L.Gp),
                     (const float*)F(L.dbp), cls, batch, Sb, C, K, (int64_t)K * 2 * C, grads);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t dvt_depth_clip_work_floats(int64_t n) { return n < 1 ? -1 : (n + kClipBlock - 1) / kClipBlock; }

extern "C" int dvt_depth_clip_grad_norm(float* grads, int64_t n, float max_norm, float* work, float* out, void* stream) {
  if (!grads || !work || !out || n < 1 || n >= (1LL << 40) || !(max_norm > 0.f)) return DVT_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const int P = (int)((n + kClipBlock - 1) / kClipBlock);
  hipLaunchKernelGGL(depth_sumsq_kernel, dim3(P), dim3(256), 0, s, (const float*)grads, n, work);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(depth_clip_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)work, P, max_norm, out);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(depth_scale_kernel, dim3(dvt_cdiv(n, 256)), dim3(256), 0, s, grads, n, (const float*)out);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t dvt_depth_eval_work_bytes(int out_h, int out_w) {
  if (out_h < 1 || out_w < 1 || (int64_t)out_h * out_w >= (1LL << 30)) return -1;
  return (int64_t)(((int64_t)out_h * out_w + kLossPix - 1) / kLossPix) * kEvalSums * 8;
}

extern "C" int dvt_depth_eval_image(const float* d0, const float* d1, int uh, int uw, const float* gt, int out_h, int out_w,
                                    float min_depth, float max_depth, int crop_y0, int crop_y1, int crop_x0, int crop_x1,
                                    float* pred, double* row, void* work, void* stream) {
  if (!d0 || !gt || !row || !work || uh < 1 || uw < 1 || out_h < 1 || out_w < 1 ||
      (int64_t)out_h * out_w >= (1LL << 30) || !(min_depth < max_depth))
    return DVT_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const int P = (out_h * out_w + kLossPix - 1) / kLossPix;
  hipLaunchKernelGGL(depth_eval_kernel, dim3(P), dim3(256), 0, s, d0, d1, uh, uw, gt, out_h, out_w, min_depth, max_depth,
                     crop_y0, crop_y1, crop_x0, crop_x1, pred, (double*)work);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(depth_eval_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)work, P, row);
  DVT_CHECK_LAUNCH();
  return 0;
}
