// dvt_video.hip -- the per-frame kernels of the feature-video demo (include/dvt_video.h): apply the bases and centres
// fitted on frame 0 to a frame's features in ONE pass over them, per-frame column ranges, the softmax-of-norm map, the
// token-resolution uint8 pictures and Pillow's 8-bit bicubic resize.
//
// The only kernel that touches the features (78 MB per frame at 120 x 211 x 768) is k_apply: a wave holds four rows in
// registers and forms every projection column, the row norm and the K cosine similarities from them, so the features are
// read once for all pictures.  Everything after it works on [n, m] projections (1.3 MB) or uint8 pictures.  Row-wise dot
// products accumulate in fp64 in a fixed order (a lane's channels in ascending order, then the xor butterfly); single fp32
// operations use the __f*_rn intrinsics so that none is contracted into an FMA.
#include "dvt_common.h"
#include "../../include/dvt_video.h"

#include <math.h>

namespace {

constexpr int kNC = DVT_VIS_MAX_C / 64;  // channel slots of a lane
constexpr int kRowsPerWave = 4;
constexpr int kColBlock = 8;             // projection columns accumulated at once
constexpr int kMaxDim = 16384;           // picture sides of the resize

bool shape_ok(int n, int C) {
  return n >= 1 && n <= DVT_VIS_MAX_ROWS && C >= 64 && C <= DVT_VIS_MAX_C && C % 64 == 0;
}

// (uint8) (v * 255) as numpy truncates a float32 in [0, 255]; NaN and negatives 0, above 255: 255
__device__ __forceinline__ uint8_t to_u8(float v) {
  const float f = __fmul_rn(v, 255.0f);
  if (f >= 255.0f) return 255;
  return f > 0.0f ? (uint8_t)(int)f : (uint8_t)0;
}

__device__ __forceinline__ float affine(float v, float s, float o) { return __fadd_rn(__fmul_rn(s, v), o); }

__device__ __forceinline__ float minmax_norm(float v, float lo, float hi) {
  return __fdiv_rn(__fsub_rn(v, lo), __fsub_rn(hi, lo));
}

// ================================================================================================================ apply
__global__ void __launch_bounds__(256) k_apply(const float* __restrict__ x, int n, int C, const float* __restrict__ M, int m,
                                               const float* __restrict__ centers, int K, float* __restrict__ P,
                                               float* __restrict__ norms, int32_t* __restrict__ labels) {
  __shared__ double s_cnorm[DVT_VIS_MAX_K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nc = C / 64;
  if (centers != nullptr) {  // centre norms exactly as dvt_vis_kmeans forms them
    for (int k = wave; k < K; k += 4) {
      const float* c = centers + (int64_t)k * C;
      double s = 0.0;
      for (int j = lane; j < C; j += 64) s += (double)c[j] * (double)c[j];
      s = wave_sum_f64(s);
      if (lane == 0) s_cnorm[k] = sqrt(s);
    }
  }
  __syncthreads();
  const int row0 = (blockIdx.x * 4 + wave) * kRowsPerWave;
  if (row0 >= n) return;

  float xv[kRowsPerWave][kNC];
  double xn[kRowsPerWave];
#pragma unroll
  for (int r = 0; r < kRowsPerWave; ++r) {
    const bool live = row0 + r < n;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < kNC; ++j) {
      xv[r][j] = (live && j < nc) ? x[(int64_t)(row0 + r) * C + j * 64 + lane] : 0.0f;
      s += (double)xv[r][j] * (double)xv[r][j];
    }
    xn[r] = sqrt(wave_sum_f64(s));
    if (live && norms != nullptr && lane == 0) norms[row0 + r] = (float)xn[r];
  }

  for (int c0 = 0; c0 < m; c0 += kColBlock) {
    double acc[kRowsPerWave][kColBlock];
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r)
#pragma unroll
      for (int c = 0; c < kColBlock; ++c) acc[r][c] = 0.0;
#pragma unroll
    for (int j = 0; j < kNC; ++j) {
      if (j < nc) {
        const float* mr = M + (int64_t)(j * 64 + lane) * m + c0;
#pragma unroll
        for (int c = 0; c < kColBlock; ++c) {
          const double w = c0 + c < m ? (double)mr[c] : 0.0;
#pragma unroll
          for (int r = 0; r < kRowsPerWave; ++r) acc[r][c] += (double)xv[r][j] * w;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
      float mine = 0.0f;
#pragma unroll
      for (int c = 0; c < kColBlock; ++c) {
        const double v = wave_sum_f64(acc[r][c]);
        if (lane == c) mine = (float)v;
      }
      if (lane < kColBlock && c0 + lane < m && row0 + r < n) P[(int64_t)(row0 + r) * m + c0 + lane] = mine;
    }
  }

  if (centers != nullptr) {
    int best[kRowsPerWave];
    double best_sim[kRowsPerWave];
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
      best[r] = 0;
      best_sim[r] = 0.0;
    }
    for (int k = 0; k < K; ++k) {
      double d[kRowsPerWave];
#pragma unroll
      for (int r = 0; r < kRowsPerWave; ++r) d[r] = 0.0;
#pragma unroll
      for (int j = 0; j < kNC; ++j) {
        if (j < nc) {
          const double cv = (double)centers[(int64_t)k * C + j * 64 + lane];
#pragma unroll
          for (int r = 0; r < kRowsPerWave; ++r) d[r] += (double)xv[r][j] * cv;
        }
      }
      const double cn = s_cnorm[k];
#pragma unroll
      for (int r = 0; r < kRowsPerWave; ++r) {
        const double dot = wave_sum_f64(d[r]);
        const double den = xn[r] * cn;
        const double sim = den > 0.0 ? dot / den : 0.0;
        if (k == 0 || sim > best_sim[r]) {
          best[r] = k;
          best_sim[r] = sim;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r)
      if (lane == 0 && row0 + r < n) labels[row0 + r] = best[r];
  }
}

// ================================================================================================================ ranges
// workgroup c < m: column c of P; workgroup m: the affine image of column affine_col
__global__ void __launch_bounds__(1024) k_col_range(const float* __restrict__ P, int n, int m, float* __restrict__ range,
                                                    int affine_col, float s, float o, float* __restrict__ affine_range) {
  __shared__ float slo[16], shi[16];
  const bool aff = (int)blockIdx.x == m;
  const int col = aff ? affine_col : (int)blockIdx.x;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    float v = P[(int64_t)i * m + col];
    if (aff) v = affine(v, s, o);
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, w, 64));
    hi = fmaxf(hi, __shfl_xor(hi, w, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    slo[threadIdx.x >> 6] = lo;
    shi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 16; ++i) {
      lo = fminf(lo, slo[i]);
      hi = fmaxf(hi, shi[i]);
    }
    if (aff) {
      affine_range[0] = lo;
      affine_range[1] = hi;
    } else {
      range[col] = lo;
      range[m + col] = hi;
    }
  }
}

// one workgroup (n <= DVT_VIS_MAX_ROWS values, 256 KB at most: they stay in the cache between the passes); p is parked in
// `out`, every element by the thread that reads it again
__global__ void __launch_bounds__(1024) k_softmax_norm(const float* __restrict__ norms, int n, float temp,
                                                       float* __restrict__ out) {
  __shared__ double redd[16];
  __shared__ float redlo[16], redhi[16];
  const int tid = threadIdx.x;
  float hi = -INFINITY;
  for (int i = tid; i < n; i += 1024) hi = fmaxf(hi, norms[i]);
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) hi = fmaxf(hi, __shfl_xor(hi, w, 64));
  if ((tid & 63) == 0) redhi[tid >> 6] = hi;
  __syncthreads();
  float vmax = redhi[0];
  for (int i = 1; i < 16; ++i) vmax = fmaxf(vmax, redhi[i]);
  const double dt = (double)temp, tmax = (double)vmax / dt;
  double sum = 0.0;
  for (int i = tid; i < n; i += 1024) sum += exp((double)norms[i] / dt - tmax);
  sum = wave_sum_f64(sum);
  if ((tid & 63) == 0) redd[tid >> 6] = sum;
  __syncthreads();
  double total = 0.0;
  for (int i = 0; i < 16; ++i) total += redd[i];
  float plo = INFINITY, phi = -INFINITY;
  for (int i = tid; i < n; i += 1024) {
    const float p = (float)(exp((double)norms[i] / dt - tmax) / total);
    out[i] = p;
    plo = fminf(plo, p);
    phi = fmaxf(phi, p);
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    plo = fminf(plo, __shfl_xor(plo, w, 64));
    phi = fmaxf(phi, __shfl_xor(phi, w, 64));
  }
  __syncthreads();  // redhi was read above
  if ((tid & 63) == 0) {
    redlo[tid >> 6] = plo;
    redhi[tid >> 6] = phi;
  }
  __syncthreads();
  plo = redlo[0];
  phi = redhi[0];
  for (int i = 1; i < 16; ++i) {
    plo = fminf(plo, redlo[i]);
    phi = fmaxf(phi, redhi[i]);
  }
  for (int i = tid; i < n; i += 1024) out[i] = minmax_norm(out[i], plo, phi);
}

__global__ void __launch_bounds__(256) k_threshold(const float* __restrict__ P, int n, int m, int col, float s, float o,
                                                   float t, uint8_t* __restrict__ mask) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) mask[i] = affine(P[(int64_t)i * m + col], s, o) > t ? 1 : 0;
}

// ================================================================================================================ pictures
__global__ void __launch_bounds__(256) k_picture_rgb(const float* __restrict__ P, int n, int m, int col0,
                                                     const float* __restrict__ range, const uint8_t* __restrict__ mask,
                                                     uint8_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float keep = mask == nullptr ? 1.0f : (float)mask[i];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = minmax_norm(P[(int64_t)i * m + col0 + c], range[col0 + c], range[m + col0 + c]);
    if (mask != nullptr) v = __fmul_rn(v, keep);
    out[(int64_t)i * 3 + c] = to_u8(v);
  }
}

__global__ void __launch_bounds__(256) k_picture_scalar(const float* __restrict__ src, int n, int stride, int col, int aff,
                                                        float s, float o, const float* __restrict__ range,
                                                        int range_stride, const uint8_t* __restrict__ table,
                                                        uint8_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float v = src[(int64_t)i * stride + col];
  if (aff) v = affine(v, s, o);
  if (range != nullptr) v = minmax_norm(v, range[0], range[range_stride]);
  uint8_t r = 0, g = 0, b = 0;
  if (v == v) {  // matplotlib: x * 256 truncated, below 0 the first entry, from 1 on the last
    const float f = __fmul_rn(v, 256.0f);
    const int e = f >= 255.0f ? 255 : (f > 0.0f ? (int)f : 0);
    r = table[e * 3 + 0];
    g = table[e * 3 + 1];
    b = table[e * 3 + 2];
  }
  out[(int64_t)i * 3 + 0] = r;
  out[(int64_t)i * 3 + 1] = g;
  out[(int64_t)i * 3 + 2] = b;
}

__global__ void __launch_bounds__(256) k_picture_labels(const int32_t* __restrict__ labels, int n,
                                                        const uint8_t* __restrict__ table, int K, uint8_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int l = labels[i];
  const bool ok = l >= 0 && l < K;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[(int64_t)i * 3 + c] = ok ? table[l * 3 + c] : (uint8_t)0;
}

__global__ void __launch_bounds__(256) k_denorm_u8(const float* __restrict__ img, int64_t pixels, const float* __restrict__ mean,
                                                   const float* __restrict__ std, uint8_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = __fdiv_rn(__fsub_rn(img[c * pixels + p], mean[c]), std[c]);
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    out[p * 3 + c] = to_u8(v);
  }
}

// ================================================================================================================ resize
// One pass of Pillow's 8-bit resample along one axis.  src [images, len_in, inner] -> dst [images, len_out, inner] bytes
// (horizontal: the axis is x, outer = the rows, inner = 3; vertical: the axis is y, outer = 1, inner = 3 W): one thread per
// output byte.
__global__ void __launch_bounds__(256) k_resample(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t outer,
                                                  int len_in, int len_out, int inner, const int32_t* __restrict__ bounds,
                                                  const int32_t* __restrict__ coef, int taps) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= outer * len_out * inner) return;
  const int c = (int)(idx % inner);
  const int xo = (int)((idx / inner) % len_out);
  const int64_t line = idx / ((int64_t)inner * len_out);
  const int first = bounds[2 * xo];
  int cnt = bounds[2 * xo + 1];
  cnt = cnt < 0 ? 0 : (cnt > taps ? taps : cnt);
  const uint8_t* sp = src + line * len_in * inner + c;
  const int32_t* k = coef + (int64_t)xo * taps;
  uint32_t acc = 1u << 21;
  for (int t = 0; t < cnt; ++t) {
    int xi = first + t;
    xi = xi < 0 ? 0 : (xi >= len_in ? len_in - 1 : xi);
    acc += (uint32_t)sp[(int64_t)xi * inner] * (uint32_t)k[t];
  }
  const int32_t v = (int32_t)acc >> 22;
  dst[idx] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

}  // namespace

// =========================================================================================================== C ABI
extern "C" {

int dvt_video_apply(const float* x, int n, int C, const float* M, int m, const float* centers, int K, float* P, float* norms,
                    int32_t* labels, void* stream) {
  if (x == nullptr || M == nullptr || P == nullptr || !shape_ok(n, C) || m < 1 || m > DVT_VIDEO_MAX_M ||
      ((centers == nullptr) != (labels == nullptr)))
    return DVT_E_BADARG;
  if (centers != nullptr && (K < 1 || K > DVT_VIS_MAX_K)) return DVT_E_BADARG;
  hipLaunchKernelGGL(k_apply, dim3(dvt_cdiv(n, 4 * kRowsPerWave)), dim3(256), 0, static_cast<hipStream_t>(stream), x, n, C, M,
                     m, centers, K, P, norms, labels);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_video_col_range(const float* P, int n, int m, float* range, int affine_col, float s, float o, float* affine_range,
                        void* stream) {
  if (P == nullptr || range == nullptr || n < 1 || n > DVT_VIS_MAX_ROWS || m < 1 || m > DVT_VIDEO_MAX_M || affine_col >= m ||
      (affine_col >= 0 && affine_range == nullptr))
    return DVT_E_BADARG;
  hipLaunchKernelGGL(k_col_range, dim3(m + (affine_col >= 0 ? 1 : 0)), dim3(1024), 0, static_cast<hipStream_t>(stream), P, n, m,
                     range, affine_col, s, o, affine_range);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_video_softmax_norm_map(const float* norms, int n, float temp, float* out, void* stream) {
  if (norms == nullptr || out == nullptr || n < 1 || n > DVT_VIS_MAX_ROWS || !(temp > 0.0f)) return DVT_E_BADARG;
  hipLaunchKernelGGL(k_softmax_norm, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), norms, n, temp, out);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_video_threshold_mask(const float* P, int n, int m, int col, float s, float o, float t, uint8_t* mask, void* stream) {
  if (P == nullptr || mask == nullptr || n < 1 || n > DVT_VIS_MAX_ROWS || m < 1 || m > DVT_VIDEO_MAX_M || col < 0 || col >= m)
    return DVT_E_BADARG;
  hipLaunchKernelGGL(k_threshold, dim3(dvt_cdiv(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), P, n, m, col, s, o, t,
                     mask);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_video_picture_rgb(const float* P, int n, int m, int col0, const float* range, const uint8_t* mask, uint8_t* out,
                          void* stream) {
  if (P == nullptr || range == nullptr || out == nullptr || n < 1 || n > DVT_VIS_MAX_ROWS || m < 3 || m > DVT_VIDEO_MAX_M ||
      col0 < 0 || col0 + 3 > m)
    return DVT_E_BADARG;
  hipLaunchKernelGGL(k_picture_rgb, dim3(dvt_cdiv(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), P, n, m, col0, range,
                     mask, out);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_video_picture_scalar(const float* v, int n, int stride, int col, int affine, float s, float o, const float* range,
                             int range_stride, const uint8_t* table, uint8_t* out, void* stream) {
  if (v == nullptr || table == nullptr || out == nullptr || n < 1 || n > DVT_VIS_MAX_ROWS || stride < 1 ||
      stride > DVT_VIDEO_MAX_M || col < 0 || col >= stride || (range != nullptr && (range_stride < 1 || range_stride > DVT_VIDEO_MAX_M)))
    return DVT_E_BADARG;
  hipLaunchKernelGGL(k_picture_scalar, dim3(dvt_cdiv(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), v, n, stride, col,
                     affine, s, o, range, range_stride, table, out);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_video_picture_labels(const int32_t* labels, int n, const uint8_t* table, int K, uint8_t* out, void* stream) {
  if (labels == nullptr || table == nullptr || out == nullptr || n < 1 || n > DVT_VIS_MAX_ROWS || K < 1 || K > DVT_VIS_MAX_K)
    return DVT_E_BADARG;
  hipLaunchKernelGGL(k_picture_labels, dim3(dvt_cdiv(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), labels, n, table,
                     K, out);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_video_denorm_u8(const float* img, int H, int W, const float* mean, const float* std, uint8_t* out, void* stream) {
  if (img == nullptr || mean == nullptr || std == nullptr || out == nullptr || H < 1 || W < 1 || H > kMaxDim || W > kMaxDim)
    return DVT_E_BADARG;
  const int64_t pixels = (int64_t)H * W;
  hipLaunchKernelGGL(k_denorm_u8, dim3(dvt_cdiv(pixels, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), img, pixels, mean,
                     std, out);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_video_resize_bicubic_u8(const uint8_t* src, int images, int h, int w, uint8_t* dst, int H, int W,
                                const int32_t* xbounds, const int32_t* xcoef, int xtaps, const int32_t* ybounds,
                                const int32_t* ycoef, int ytaps, uint8_t* tmp, void* stream) {
  if (src == nullptr || dst == nullptr || tmp == nullptr || xbounds == nullptr || xcoef == nullptr || ybounds == nullptr ||
      ycoef == nullptr || images < 1 || images > DVT_VIDEO_MAX_IMAGES || h < 1 || w < 1 || H < 1 || W < 1 || h > kMaxDim ||
      w > kMaxDim || H > kMaxDim || W > kMaxDim || xtaps < 1 || xtaps > DVT_VIDEO_MAX_TAPS || ytaps < 1 ||
      ytaps > DVT_VIDEO_MAX_TAPS)
    return DVT_E_BADARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t nh = (int64_t)images * h * W * 3, nv = (int64_t)images * H * W * 3;
  if (nh > (int64_t)INT32_MAX * 128 || nv > (int64_t)INT32_MAX * 128) return DVT_E_BADARG;
  hipLaunchKernelGGL(k_resample, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, s, src, tmp, (int64_t)images * h, w, W, 3,
                     xbounds, xcoef, xtaps);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_resample, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, (const uint8_t*)tmp, dst, (int64_t)images, h,
                     H, 3 * W, ybounds, ycoef, ytaps);
  DVT_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
