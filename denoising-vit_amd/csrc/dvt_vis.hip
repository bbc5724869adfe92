// dvt_vis.hip -- feature-map visualisation (include/dvt_vis.h): robust PCA colours, norm / similarity maps, cosine
// k-means and the composition of the panels into one canvas.
//
// Everything here is small dense work on maps of a few thousand rows: the one piece with real arithmetic is the C x C
// covariance (1.6 GFLOP at 1369 x 768), done as a 64 x 64-tiled fp32 FMA product whose k-order is fixed.  Row-wise dot
// products (norms, cosines, projections, k-means similarities) accumulate in fp64 and round once; cross-workgroup
// reductions go through per-workgroup partial records that a later launch adds up in index order.  No kernel waits for
// another workgroup.
#include "dvt_common.h"
#include "../../include/dvt_vis.h"

#include <math.h>

namespace {

constexpr int kAssignRows = 32;  // rows per workgroup of the k-means assignment
constexpr int kScratchBytes = 1024;

inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

struct VisLayout {
  int64_t mean, cov, y0, y1, q, tmp, scratch, km_centers, km_cnorm, km_labels, km_shift, km_inp, km_state, km_inertia, total;
};

bool shape_ok(int n, int C) {
  return n >= 1 && n <= DVT_VIS_MAX_ROWS && C >= 64 && C <= DVT_VIS_MAX_C && C % 64 == 0;
}

VisLayout vis_layout(int n, int C, int K, int R) {
  VisLayout L;
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    const int64_t at = o;
    o += align256(bytes);
    return at;
  };
  L.scratch = take(kScratchBytes);  // first: its place does not depend on C
  L.tmp = take((int64_t)n * 4);
  L.mean = take((int64_t)C * 8 + 8);  // double [C], then the selected-row count (int)
  L.cov = take((int64_t)C * C * 4);
  L.y0 = take((int64_t)C * 3 * 4);
  L.y1 = take((int64_t)C * 3 * 4);
  L.q = take((int64_t)C * 3 * 4);
  L.km_centers = take((int64_t)R * K * C * 4);
  L.km_cnorm = take((int64_t)R * K * 8);
  L.km_labels = take((int64_t)R * n * 4);
  L.km_shift = take((int64_t)R * (C / 64) * 8);
  L.km_inp = take((int64_t)R * dvt_cdiv(n, kAssignRows) * 8);
  L.km_state = take((int64_t)R * 4 * 4);
  L.km_inertia = take((int64_t)R * 8);
  L.total = o;
  return L;
}

// ---- block-wide reductions in a fixed order (blockDim.x a multiple of 64, at most 1024) -------------------------------
__device__ double block_sum_d(double v, double* red /* [16] */) {
  v = wave_sum_f64(v);
  __syncthreads();  // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  const int nw = blockDim.x >> 6;
  for (int i = 0; i < nw; ++i) s += red[i];
  return s;
}

__device__ int block_sum_i(int v, int* red /* [16] */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
  const int nw = blockDim.x >> 6;
  for (int i = 0; i < nw; ++i) s += red[i];
  return s;
}

// (value, row) records: the smaller value wins, the lower row on equal values; sign = -1 turns it into a maximum
struct ValRow {
  double v;
  int row;
};
__device__ __forceinline__ ValRow vr_better(ValRow a, ValRow b) {
  if (b.row < 0) return a;
  if (a.row < 0) return b;
  if (b.v < a.v || (b.v == a.v && b.row < a.row)) return b;
  return a;
}
__device__ ValRow block_best(ValRow r, double* redv /* [16] */, int* redi /* [16] */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ValRow other;
    other.v = __shfl_xor(r.v, o, 64);
    other.row = __shfl_xor(r.row, o, 64);
    r = vr_better(r, other);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    redv[threadIdx.x >> 6] = r.v;
    redi[threadIdx.x >> 6] = r.row;
  }
  __syncthreads();
  ValRow best;
  best.v = 0.0;
  best.row = -1;
  const int nw = blockDim.x >> 6;
  for (int i = 0; i < nw; ++i) {
    ValRow c;
    c.v = redv[i];
    c.row = redi[i];
    best = vr_better(best, c);
  }
  return best;
}

// ======================================================================================================= PCA
// column means over the selected rows (fp64), 64 columns per workgroup, 16 row groups
__global__ void __launch_bounds__(1024) k_colmean(const float* __restrict__ x, const uint8_t* __restrict__ mask, int n, int C,
                                                  double* __restrict__ mean, int* __restrict__ count) {
  __shared__ double part[16][64];
  __shared__ int cnts[16];
  const int col = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + col;
  double acc = 0.0;
  int cnt = 0;
  for (int r = rg; r < n; r += 16) {
    if (mask == nullptr || mask[r] != 0) {
      acc += (double)x[(int64_t)r * C + c];
      ++cnt;
    }
  }
  part[rg][col] = acc;
  if (col == 0) cnts[rg] = cnt;
  __syncthreads();
  if (rg == 0) {
    double s = 0.0;
    int total = 0;
    for (int i = 0; i < 16; ++i) {
      s += part[i][col];
      total += cnts[i];
    }
    mean[c] = total > 0 ? s / (double)total : 0.0;
    if (blockIdx.x == 0 && col == 0) *count = total;
  }
}

// cov[i][j] = sum_r (x[r][i] - mean[i]) (x[r][j] - mean[j]) / (count - 1): 64 x 64 tiles of the upper triangle, mirrored
__global__ void __launch_bounds__(256) k_cov(const float* __restrict__ x, const uint8_t* __restrict__ mask, int n, int C,
                                             const double* __restrict__ mean, const int* __restrict__ count,
                                             float* __restrict__ cov) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  __shared__ __attribute__((aligned(16))) float A[16][64];
  __shared__ __attribute__((aligned(16))) float B[16][64];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int lr = tid >> 4, lc = (tid & 15) * 4;  // this thread's float4 of a 16 x 64 chunk
  float ma[4], mb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ma[i] = (float)mean[bi * 64 + lc + i];
    mb[i] = (float)mean[bj * 64 + lc + i];
  }
  float acc[4][4] = {};
  for (int r0 = 0; r0 < n; r0 += 16) {
    const int r = r0 + lr;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (r < n && (mask == nullptr || mask[r] != 0)) {
      a = *reinterpret_cast<const float4*>(x + (int64_t)r * C + bi * 64 + lc);
      b = *reinterpret_cast<const float4*>(x + (int64_t)r * C + bj * 64 + lc);
      a.x -= ma[0]; a.y -= ma[1]; a.z -= ma[2]; a.w -= ma[3];
      b.x -= mb[0]; b.y -= mb[1]; b.z -= mb[2]; b.w -= mb[3];
    }
    __syncthreads();
    *reinterpret_cast<float4*>(&A[lr][lc]) = a;
    *reinterpret_cast<float4*>(&B[lr][lc]) = b;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float4 av = *reinterpret_cast<const float4*>(&A[k][ty * 4]);
      const float4 bv = *reinterpret_cast<const float4*>(&B[k][tx * 4]);
      const float aa[4] = {av.x, av.y, av.z, av.w}, bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(aa[i], bb[j], acc[i][j]);
    }
  }
  const int cnt = *count;
  const float scale = cnt > 1 ? 1.0f / (float)(cnt - 1) : 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gi = bi * 64 + ty * 4 + i, gj = bj * 64 + tx * 4 + j;
      const float v = acc[i][j] * scale;
      cov[(int64_t)gi * C + gj] = v;
      if (bi != bj) cov[(int64_t)gj * C + gi] = v;
    }
}

// the fixed dense start basis: a hash of the element index, in [-1, 1)
__device__ __forceinline__ float vis_start(int c, int j) {
  uint32_t h = (uint32_t)(c * 3 + j + 1) * 2654435761u;
  h ^= h >> 15;
  h *= 2246822519u;
  h ^= h >> 13;
  return (float)(h >> 8) * (1.0f / 8388608.0f) - 1.0f;
}

// modified Gram-Schmidt of the three columns of Y [C][3] held in LDS (every workgroup does the same arithmetic)
__device__ void mgs3(float* Y, int C, double* red) {
  for (int j = 0; j < 3; ++j) {
    for (int p = 0; p < j; ++p) {
      double d = 0.0;
      for (int c = threadIdx.x; c < C; c += blockDim.x) d += (double)Y[c * 3 + p] * (double)Y[c * 3 + j];
      d = block_sum_d(d, red);
      const float df = (float)d;
      for (int c = threadIdx.x; c < C; c += blockDim.x) Y[c * 3 + j] = fmaf(-df, Y[c * 3 + p], Y[c * 3 + j]);
      __syncthreads();
    }
    double s = 0.0;
    for (int c = threadIdx.x; c < C; c += blockDim.x) s += (double)Y[c * 3 + j] * (double)Y[c * 3 + j];
    s = block_sum_d(s, red);
    const float inv = s > 0.0 ? (float)(1.0 / sqrt(s)) : 0.0f;
    for (int c = threadIdx.x; c < C; c += blockDim.x) Y[c * 3 + j] *= inv;
    __syncthreads();
  }
}

// one step: Q = orth(Yin) (the start basis when first), Yout[rows of this workgroup] = cov Q; workgroup 0 keeps Q
__global__ void __launch_bounds__(256) k_pca_iter(const float* __restrict__ cov, const float* __restrict__ yin, int first,
                                                  int C, float* __restrict__ yout, float* __restrict__ qout) {
  __shared__ float Y[DVT_VIS_MAX_C * 3];
  __shared__ double red[16];
  for (int i = threadIdx.x; i < C * 3; i += blockDim.x) Y[i] = first ? vis_start(i / 3, i % 3) : yin[i];
  __syncthreads();
  mgs3(Y, C, red);
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < C * 3; i += blockDim.x) qout[i] = Y[i];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int rr = wave; rr < 64; rr += 4) {
    const int row = blockIdx.x * 64 + rr;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int k = lane; k < C; k += 64) {
      const float v = cov[(int64_t)row * C + k];
      a0 = fmaf(v, Y[k * 3 + 0], a0);
      a1 = fmaf(v, Y[k * 3 + 1], a1);
      a2 = fmaf(v, Y[k * 3 + 2], a2);
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    a2 = wave_sum(a2);
    if (lane == 0) {
      yout[row * 3 + 0] = a0;
      yout[row * 3 + 1] = a1;
      yout[row * 3 + 2] = a2;
    }
  }
}

// evals = Rayleigh quotients q_j . (cov q_j), basis = orth(y) with the sign rule
__global__ void __launch_bounds__(256) k_pca_finish(const float* __restrict__ y, const float* __restrict__ q, int C,
                                                    const int* __restrict__ count, float* __restrict__ basis,
                                                    float* __restrict__ evals) {
  __shared__ float Y[DVT_VIS_MAX_C * 3];
  __shared__ double red[16];
  __shared__ double redv[16];
  __shared__ int redi[16];
  if (*count < 2) {
    for (int i = threadIdx.x; i < C * 3; i += blockDim.x) basis[i] = 0.0f;
    if (threadIdx.x < 3) evals[threadIdx.x] = 0.0f;
    return;
  }
  for (int i = threadIdx.x; i < C * 3; i += blockDim.x) Y[i] = y[i];
  __syncthreads();
  for (int j = 0; j < 3; ++j) {
    double d = 0.0;
    for (int c = threadIdx.x; c < C; c += blockDim.x) d += (double)q[c * 3 + j] * (double)Y[c * 3 + j];
    d = block_sum_d(d, red);
    if (threadIdx.x == 0) evals[j] = (float)d;
  }
  mgs3(Y, C, red);
  for (int j = 0; j < 3; ++j) {
    ValRow r;
    r.v = 0.0;
    r.row = -1;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {  // largest magnitude = smallest negated magnitude, lowest index
      ValRow t;
      t.v = -fabs((double)Y[c * 3 + j]);
      t.row = c;
      r = vr_better(r, t);
    }
    r = block_best(r, redv, redi);
    const float sgn = (r.row >= 0 && Y[r.row * 3 + j] < 0.0f) ? -1.0f : 1.0f;
    for (int c = threadIdx.x; c < C; c += blockDim.x) basis[c * 3 + j] = sgn * Y[c * 3 + j];
    __syncthreads();
  }
}

// ======================================================================================================= row kernels
// one wave per row; mode 0: out[n][3] = x basis (optionally range-normalised); 1: out[n] = |x|; 2: out[n] = cos(x, x[center])
__global__ void __launch_bounds__(256) k_rows(const float* __restrict__ x, int n, int C, int mode, const float* __restrict__ basis,
                                              const float* __restrict__ rgb_min, const float* __restrict__ rgb_max, int center,
                                              float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float* xr = x + (int64_t)row * C;
  if (mode == 0) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int k = lane; k < C; k += 64) {
      const double v = (double)xr[k];
      a0 += v * (double)basis[k * 3 + 0];
      a1 += v * (double)basis[k * 3 + 1];
      a2 += v * (double)basis[k * 3 + 2];
    }
    a0 = wave_sum_f64(a0);
    a1 = wave_sum_f64(a1);
    a2 = wave_sum_f64(a2);
    if (lane < 3) {
      float v = (float)(lane == 0 ? a0 : (lane == 1 ? a1 : a2));
      if (rgb_min != nullptr) {
        v = (v - rgb_min[lane]) / (rgb_max[lane] - rgb_min[lane]);
        v = fminf(fmaxf(v, 0.0f), 1.0f);  // (NaN -> 0)
      }
      out[(int64_t)row * 3 + lane] = v;
    }
  } else if (mode == 1) {
    double s = 0.0;
    for (int k = lane; k < C; k += 64) s += (double)xr[k] * (double)xr[k];
    s = wave_sum_f64(s);
    if (lane == 0) out[row] = (float)sqrt(s);
  } else {
    const float* xc = x + (int64_t)center * C;
    double d = 0.0, s = 0.0, sc = 0.0;
    for (int k = lane; k < C; k += 64) {
      const double a = (double)xr[k], b = (double)xc[k];
      d += a * b;
      s += a * a;
      sc += b * b;
    }
    d = wave_sum_f64(d);
    s = wave_sum_f64(s);
    sc = wave_sum_f64(sc);
    if (lane == 0) out[row] = (float)(d / (sqrt(s) * sqrt(sc)));
  }
}

// out = (v - min) / (max - min + eps) over one array (one workgroup); out[center] = -1 when center >= 0
__global__ void __launch_bounds__(1024) k_minmax_norm(const float* __restrict__ v, int n, float eps, int center,
                                                      float* __restrict__ out) {
  __shared__ double redv[16];
  __shared__ int redi[16];
  ValRow lo, hi;
  lo.v = hi.v = 0.0;
  lo.row = hi.row = -1;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    ValRow t;
    t.v = (double)v[i];
    t.row = i;
    lo = vr_better(lo, t);
    t.v = -t.v;
    hi = vr_better(hi, t);
  }
  lo = block_best(lo, redv, redi);
  hi = block_best(hi, redv, redi);
  const float mn = (float)lo.v, mx = (float)(-hi.v);
  const float den = (mx - mn) + eps;
  for (int i = threadIdx.x; i < n; i += blockDim.x) out[i] = (i == center) ? -1.0f : (v[i] - mn) / den;
}

__global__ void __launch_bounds__(1024) k_fg_mask(const float* __restrict__ colors, int n, float thresh,
                                                  uint8_t* __restrict__ mask) {
  __shared__ double redv[16];
  __shared__ int redi[16];
  ValRow lo, hi;
  lo.v = hi.v = 0.0;
  lo.row = hi.row = -1;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    ValRow t;
    t.v = (double)colors[(int64_t)i * 3];
    t.row = i;
    lo = vr_better(lo, t);
    t.v = -t.v;
    hi = vr_better(hi, t);
  }
  lo = block_best(lo, redv, redi);
  hi = block_best(hi, redv, redi);
  const float mn = (float)lo.v, mx = (float)(-hi.v);
  for (int i = threadIdx.x; i < n; i += blockDim.x)
    mask[i] = ((colors[(int64_t)i * 3] - mn) / (mx - mn) < thresh) ? 1 : 0;
}

// ======================================================================================================= robust range
// order-preserving integer image of a double
__device__ __forceinline__ uint64_t key_of(double v) {
  if (v == 0.0) v = 0.0;  // -0.0 and +0.0 are one value: one key
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// The value of rank `rank` (0-based, ascending) among get(i) over the selected rows, by an 8-bit radix select on the
// keys, most significant digit first; *row_out = the lowest selected row that holds it.  All threads take part.
template <typename Get>
__device__ double radix_select(Get get, const uint8_t* mask, int n, int rank, int* hist /* [256] */, uint64_t* bc /* [2] */,
                               double* redv, int* redi, int* row_out) {
  uint64_t prefix = 0, pmask = 0;
  for (int pass = 7; pass >= 0; --pass) {
    const int shift = pass * 8;
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      if (mask != nullptr && mask[i] == 0) continue;
      const uint64_t k = key_of(get(i));
      if ((k & pmask) == prefix) atomicAdd(&hist[(int)((k >> shift) & 255u)], 1);  // integer LDS counts: order-free
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int cum = 0, b = 0;
      for (; b < 255; ++b) {
        if (rank < cum + hist[b]) break;
        cum += hist[b];
      }
      bc[0] = prefix | ((uint64_t)b << shift);
      bc[1] = (uint64_t)(rank - cum);
    }
    __syncthreads();
    prefix = bc[0];
    rank = (int)bc[1];
    pmask |= (0xffull << shift);
  }
  ValRow r;
  r.v = 0.0;
  r.row = -1;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    if (mask != nullptr && mask[i] == 0) continue;
    if (key_of(get(i)) == prefix) {
      ValRow t;
      t.v = 0.0;
      t.row = i;
      r = vr_better(r, t);
    }
  }
  r = block_best(r, redv, redi);
  *row_out = r.row;
  return value_of(prefix);
}

struct RangeRec {  // per channel, in the scratch section
  double mn, mx, gmn, gmx, med, dev;
  int row_med, row_dev, row_mn, row_mx, row_gmn, row_gmx, inliers, count;
};

__global__ void __launch_bounds__(1024) k_robust(const float* __restrict__ colors, const uint8_t* __restrict__ mask, int n,
                                                 float m, RangeRec* __restrict__ rec) {
  __shared__ int hist[256];
  __shared__ uint64_t bc[2];
  __shared__ double redv[16];
  __shared__ int redi[16];
  const int ch = blockIdx.x;
  int cnt = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) cnt += (mask == nullptr || mask[i] != 0) ? 1 : 0;
  cnt = block_sum_i(cnt, redi);
  RangeRec out;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  out.mn = out.mx = out.med = out.dev = nan;
  out.row_med = out.row_dev = out.row_mn = out.row_mx = -1;
  out.inliers = 0;
  out.count = cnt;
  // the fall-back range: every row of this channel
  ValRow glo, ghi;
  glo.v = ghi.v = 0.0;
  glo.row = ghi.row = -1;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    ValRow t;
    t.v = (double)colors[(int64_t)i * 3 + ch];
    t.row = i;
    glo = vr_better(glo, t);
    t.v = -t.v;
    ghi = vr_better(ghi, t);
  }
  glo = block_best(glo, redv, redi);
  ghi = block_best(ghi, redv, redi);
  out.gmn = glo.v;
  out.gmx = -ghi.v;
  out.row_gmn = glo.row;
  out.row_gmx = ghi.row;
  if (cnt > 0) {
    const int rank = (cnt - 1) / 2;  // torch.median: the lower of the two middle values
    int row = -1;
    const double med =
        radix_select([&](int i) { return (double)colors[(int64_t)i * 3 + ch]; }, mask, n, rank, hist, bc, redv, redi, &row);
    out.med = med;
    out.row_med = row;
    const double dev = radix_select([&](int i) { return fabs((double)colors[(int64_t)i * 3 + ch] - med); }, mask, n, rank,
                                    hist, bc, redv, redi, &row);
    out.dev = dev;
    out.row_dev = row;
    ValRow lo, hi;
    lo.v = hi.v = 0.0;
    lo.row = hi.row = -1;
    int inl = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      if (mask != nullptr && mask[i] == 0) continue;
      const double c = (double)colors[(int64_t)i * 3 + ch];
      if (fabs(c - med) / dev < (double)m) {  // (0 / 0 and x / 0 are no inliers, as in the reference)
        ++inl;
        ValRow t;
        t.v = c;
        t.row = i;
        lo = vr_better(lo, t);
        t.v = -c;
        hi = vr_better(hi, t);
      }
    }
    inl = block_sum_i(inl, redi);
    lo = block_best(lo, redv, redi);
    hi = block_best(hi, redv, redi);
    out.inliers = inl;
    if (inl > 0) {
      out.mn = lo.v;
      out.mx = -hi.v;
      out.row_mn = lo.row;
      out.row_mx = hi.row;
    }
  }
  if (threadIdx.x == 0) rec[ch] = out;
}

__global__ void k_robust_finish(const RangeRec* __restrict__ rec, float* __restrict__ range, double* __restrict__ stats,
                                int32_t* __restrict__ rows) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const bool none = rec[0].count == 0;
  const bool fallback = !none && (rec[0].inliers == 0 || rec[1].inliers == 0 || rec[2].inliers == 0);
  double gmn = rec[0].gmn, gmx = rec[0].gmx;
  int rgmn = rec[0].row_gmn, rgmx = rec[0].row_gmx;
  for (int c = 1; c < 3; ++c) {
    if (rec[c].gmn < gmn) { gmn = rec[c].gmn; rgmn = rec[c].row_gmn; }
    if (rec[c].gmx > gmx) { gmx = rec[c].gmx; rgmx = rec[c].row_gmx; }
  }
  for (int c = 0; c < 3; ++c) {
    range[c] = (float)(fallback ? gmn : rec[c].mn);
    range[3 + c] = (float)(fallback ? gmx : rec[c].mx);
    if (stats != nullptr) {
      stats[c] = rec[c].med;
      stats[3 + c] = rec[c].dev;
    }
    if (rows != nullptr) {
      rows[c] = rec[c].row_med;
      rows[3 + c] = rec[c].row_dev;
      rows[6 + c] = fallback ? rgmn : rec[c].row_mn;
      rows[9 + c] = fallback ? rgmx : rec[c].row_mx;
    }
  }
  if (rows != nullptr) rows[12] = fallback ? 1 : 0;
}

// ======================================================================================================= k-means
struct KmPtrs {
  float* centers;    // [R][K][C]
  double* cnorm;     // [R][K]
  int32_t* labels;   // [R][n]
  double* shift;     // [R][C / 64]
  double* inp;       // [R][nblk]
  int32_t* state;    // [R][4]: done, iterations
  double* inertia;   // [R]
};

__global__ void __launch_bounds__(256) k_km_init(const float* __restrict__ x, int n, int C, int K,
                                                 const int32_t* __restrict__ init_rows, const float* __restrict__ init_centers,
                                                 KmPtrs p) {
  const int k = blockIdx.x, r = blockIdx.y;
  const float* src;
  if (init_centers != nullptr) {
    src = init_centers + ((int64_t)r * K + k) * C;
  } else {
    int row = init_rows[r * K + k];
    row = row < 0 ? 0 : (row >= n ? n - 1 : row);
    src = x + (int64_t)row * C;
  }
  float* dst = p.centers + ((int64_t)r * K + k) * C;
  for (int c = threadIdx.x; c < C; c += blockDim.x) dst[c] = src[c];
  if (k == 0 && threadIdx.x == 0) {
    p.state[r * 4 + 0] = 0;
    p.state[r * 4 + 1] = 0;
    p.inertia[r] = __longlong_as_double(0x7ff8000000000000ll);
  }
}

// between iterations (one workgroup per restart): add up the records of step - 1, decide, prepare the centre norms
__global__ void __launch_bounds__(256) k_km_control(int step, int n, int C, int K, float tol, KmPtrs p) {
  const int r = blockIdx.x;
  __shared__ int s_done;
  if (threadIdx.x == 0) {
    int done = p.state[r * 4 + 0];
    if (!done && step > 0) {
      const int ncb = C / 64, nblk = (n + kAssignRows - 1) / kAssignRows;
      double shift = 0.0, inertia = 0.0;
      for (int i = 0; i < ncb; ++i) shift += p.shift[r * ncb + i];
      for (int i = 0; i < nblk; ++i) inertia += p.inp[(int64_t)r * nblk + i];
      p.state[r * 4 + 1] = step;
      p.inertia[r] = inertia;
      if (shift < (double)tol) {
        done = 1;
        p.state[r * 4 + 0] = 1;
      }
    }
    s_done = done;
  }
  __syncthreads();
  if (s_done) return;
  const int lane = threadIdx.x & 63;
  for (int k = threadIdx.x >> 6; k < K; k += 4) {
    const float* c = p.centers + ((int64_t)r * K + k) * C;
    double s = 0.0;
    for (int j = lane; j < C; j += 64) s += (double)c[j] * (double)c[j];
    s = wave_sum_f64(s);
    if (lane == 0) p.cnorm[r * K + k] = sqrt(s);
  }
}

__global__ void __launch_bounds__(256) k_km_assign(const float* __restrict__ x, int n, int C, int K, KmPtrs p) {
  const int r = blockIdx.y;
  if (p.state[r * 4 + 0]) return;
  __shared__ double part[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* cen = p.centers + (int64_t)r * K * C;
  const int nc = C / 64;
  double inertia = 0.0;
  for (int i = 0; i < kAssignRows / 4; ++i) {
    const int row = blockIdx.x * kAssignRows + i * 4 + wave;
    if (row >= n) break;
    float xv[DVT_VIS_MAX_C / 64];
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < DVT_VIS_MAX_C / 64; ++j) {
      xv[j] = j < nc ? x[(int64_t)row * C + j * 64 + lane] : 0.0f;
      s += (double)xv[j] * (double)xv[j];
    }
    const double xn = sqrt(wave_sum_f64(s));
    int best = 0;
    double best_sim = 0.0;
    for (int k = 0; k < K; ++k) {
      double d = 0.0;
#pragma unroll
      for (int j = 0; j < DVT_VIS_MAX_C / 64; ++j)
        if (j < nc) d += (double)xv[j] * (double)cen[(int64_t)k * C + j * 64 + lane];
      d = wave_sum_f64(d);
      const double den = xn * p.cnorm[r * K + k];
      const double sim = den > 0.0 ? d / den : 0.0;
      if (k == 0 || sim > best_sim) {
        best = k;
        best_sim = sim;
      }
    }
    if (lane == 0) p.labels[(int64_t)r * n + row] = best;
    inertia += 1.0 - best_sim;
  }
  if (lane == 0) part[wave] = inertia;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nblk = (n + kAssignRows - 1) / kAssignRows;
    p.inp[(int64_t)r * nblk + blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
  }
}

// new centres of 64 columns: per-label sums in LDS slots that one thread owns (4 row groups), added up in order
__global__ void __launch_bounds__(256) k_km_update(const float* __restrict__ x, int n, int C, int K, KmPtrs p) {
  const int r = blockIdx.y, cb = blockIdx.x;
  if (p.state[r * 4 + 0]) return;
  __shared__ double acc[4][DVT_VIS_MAX_K][64];
  __shared__ int cnt[4][DVT_VIS_MAX_K];
  __shared__ double red[16];
  const int col = threadIdx.x & 63, rg = threadIdx.x >> 6;
  for (int k = 0; k < K; ++k) acc[rg][k][col] = 0.0;
  if (col < K) cnt[rg][col] = 0;
  __syncthreads();
  const int32_t* lab = p.labels + (int64_t)r * n;
  for (int row = rg; row < n; row += 4) {
    const int l = lab[row];
    if (l < 0 || l >= K) continue;
    acc[rg][l][col] += (double)x[(int64_t)row * C + cb * 64 + col];
    if (col == 0) cnt[rg][l] += 1;
  }
  __syncthreads();
  double sh = 0.0;
  for (int e = threadIdx.x; e < K * 64; e += blockDim.x) {
    const int k = e >> 6, c = e & 63;
    const double s = ((acc[0][k][c] + acc[1][k][c]) + acc[2][k][c]) + acc[3][k][c];
    const int m = cnt[0][k] + cnt[1][k] + cnt[2][k] + cnt[3][k];
    float* dst = p.centers + ((int64_t)r * K + k) * C + cb * 64 + c;
    if (m > 0) {  // an empty cluster keeps its centre
      const float nv = (float)(s / (double)m);
      const double d = (double)nv - (double)*dst;
      sh += d * d;
      *dst = nv;
    }
  }
  sh = block_sum_d(sh, red);
  if (threadIdx.x == 0) p.shift[r * (C / 64) + cb] = sh;
}

__global__ void __launch_bounds__(256) k_km_select(int n, int C, int K, int R, KmPtrs p, int32_t* __restrict__ labels,
                                                   float* __restrict__ centers, double* __restrict__ inertia,
                                                   int32_t* __restrict__ iterations, int32_t* __restrict__ best_out) {
  int best = 0;
  double bi = p.inertia[0];
  for (int r = 1; r < R; ++r) {
    const double v = p.inertia[r];
    if (v < bi || (bi != bi && v == v)) {
      best = r;
      bi = v;
    }
  }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) labels[i] = p.labels[(int64_t)best * n + i];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < K * C; i += gridDim.x * blockDim.x)
    centers[i] = p.centers[(int64_t)best * K * C + i];
  if (blockIdx.x == 0 && threadIdx.x < R) {
    inertia[threadIdx.x] = p.inertia[threadIdx.x];
    iterations[threadIdx.x] = p.state[threadIdx.x * 4 + 1];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && best_out != nullptr) *best_out = best;
}

// ======================================================================================================= rendering
struct Rect {
  float* canvas;
  int ch, cw, y0, x0, H, W;
};

__device__ __forceinline__ int nearest_index(int dst, int in, int out) {
  const float scale = (float)in / (float)out;
  const int i = (int)floorf((float)dst * scale);
  return i < in - 1 ? i : in - 1;
}
__device__ __forceinline__ void bilinear_index(int dst, int in, int out, int* i0, int* i1, float* l1) {
  if (in == out) {
    *i0 = *i1 = dst;
    *l1 = 0.0f;
    return;
  }
  const float scale = (float)in / (float)out;
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.0f ? 0.0f : src;
  int a = (int)src;
  a = a < in - 1 ? a : in - 1;
  *i0 = a;
  *i1 = a < in - 1 ? a + 1 : a;
  *l1 = fminf(fmaxf(src - (float)a, 0.0f), 1.0f);
}

// one thread per pixel of the rectangle; `stride` / `plane`: element strides of a pixel / a channel of the source
template <int NCH>
__device__ __forceinline__ void sample(const float* __restrict__ map, int h, int w, int64_t stride, int64_t plane, int interp,
                                       int y, int x, int H, int W, float* out) {
  if (interp == DVT_VIS_NEAREST) {
    const int sy = nearest_index(y, h, H), sx = nearest_index(x, w, W);
#pragma unroll
    for (int c = 0; c < NCH; ++c) out[c] = map[((int64_t)sy * w + sx) * stride + c * plane];
  } else {
    int y0, y1, x0, x1;
    float ly, lx;
    bilinear_index(y, h, H, &y0, &y1, &ly);
    bilinear_index(x, w, W, &x0, &x1, &lx);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const float* m = map + c * plane;
      const float v00 = m[((int64_t)y0 * w + x0) * stride], v01 = m[((int64_t)y0 * w + x1) * stride];
      const float v10 = m[((int64_t)y1 * w + x0) * stride], v11 = m[((int64_t)y1 * w + x1) * stride];
      const float top = (1.0f - lx) * v00 + lx * v01, bot = (1.0f - lx) * v10 + lx * v11;
      out[c] = (1.0f - ly) * top + ly * bot;
    }
  }
}

__device__ __forceinline__ void put(const Rect& r, int y, int x, float cr, float cg, float cb) {
  const int64_t plane = (int64_t)r.ch * r.cw;
  const int64_t at = (int64_t)(r.y0 + y) * r.cw + (r.x0 + x);
  r.canvas[at] = cr;
  r.canvas[plane + at] = cg;
  r.canvas[2 * plane + at] = cb;
}

__global__ void __launch_bounds__(256) k_render_scalar(const float* __restrict__ map, int h, int w, int interp,
                                                       const float* __restrict__ table, int neg_red, Rect r) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)r.H * r.W) return;
  const int y = (int)(i / r.W), x = (int)(i % r.W);
  float v;
  sample<1>(map, h, w, 1, 0, interp, y, x, r.H, r.W, &v);
  if (neg_red && v < 0.0f) {
    put(r, y, x, 1.0f, 0.0f, 0.0f);
    return;
  }
  if (table == nullptr) {
    put(r, y, x, v, v, v);
    return;
  }
  const float c = fminf(fmaxf(v, 0.0f), 1.0f);
  int idx = (int)(c * 256.0f);
  idx = idx > 255 ? 255 : idx;
  put(r, y, x, table[idx * 3 + 0], table[idx * 3 + 1], table[idx * 3 + 2]);
}

__global__ void __launch_bounds__(256) k_render_rgb(const float* __restrict__ map, int h, int w, int planar, int interp, Rect r) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)r.H * r.W) return;
  const int y = (int)(i / r.W), x = (int)(i % r.W);
  float v[3];
  if (planar)
    sample<3>(map, h, w, 1, (int64_t)h * w, interp, y, x, r.H, r.W, v);
  else
    sample<3>(map, h, w, 3, 1, interp, y, x, r.H, r.W, v);
  put(r, y, x, v[0], v[1], v[2]);
}

__global__ void __launch_bounds__(256) k_render_labels(const int32_t* __restrict__ labels, int h, int w,
                                                       const float* __restrict__ table, int K, Rect r) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)r.H * r.W) return;
  const int y = (int)(i / r.W), x = (int)(i % r.W);
  const int l = labels[(int64_t)nearest_index(y, h, r.H) * w + nearest_index(x, w, r.W)];
  if (l < 0 || l >= K) {
    put(r, y, x, 0.0f, 0.0f, 0.0f);
    return;
  }
  put(r, y, x, table[l * 3 + 0], table[l * 3 + 1], table[l * 3 + 2]);
}

__global__ void __launch_bounds__(256) k_fill(Rect r, float cr, float cg, float cb) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)r.H * r.W) return;
  put(r, (int)(i / r.W), (int)(i % r.W), cr, cg, cb);
}

__global__ void __launch_bounds__(256) k_to_u8(const float* __restrict__ canvas, int64_t pixels, uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pixels) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = fminf(fmaxf(canvas[c * pixels + i], 0.0f), 1.0f) * 255.0f;
    out[i * 3 + c] = (uint8_t)(int)v;
  }
}

bool rect_ok(const void* canvas, int ch, int cw, int y0, int x0, int H, int W) {
  return canvas != nullptr && ch > 0 && cw > 0 && H > 0 && W > 0 && y0 >= 0 && x0 >= 0 && (int64_t)y0 + H <= ch &&
         (int64_t)x0 + W <= cw && ch <= 32768 && cw <= 32768;
}

}  // namespace

// =========================================================================================================== C ABI
extern "C" {

int64_t dvt_vis_workspace_bytes(int n, int C, int K, int num_init) {
  if (!shape_ok(n, C) || K < 0 || K > DVT_VIS_MAX_K || num_init < 0 || num_init > DVT_VIS_MAX_INIT) return DVT_E_BADARG;
  return vis_layout(n, C, K, num_init).total;
}

int dvt_vis_pca_basis(const float* x, const uint8_t* mask, int n, int C, int iters, float* basis, float* evals, void* work,
                      int64_t work_bytes, void* stream) {
  if (x == nullptr || basis == nullptr || evals == nullptr || work == nullptr || !shape_ok(n, C) || iters < 1 ||
      iters > DVT_VIS_MAX_ITER)
    return DVT_E_BADARG;
  const VisLayout L = vis_layout(n, C, 0, 0);
  if (work_bytes < L.total) return DVT_E_BADARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* wb = static_cast<char*>(work);
  double* mean = reinterpret_cast<double*>(wb + L.mean);
  int* count = reinterpret_cast<int*>(wb + L.mean + (int64_t)C * 8);
  float* cov = reinterpret_cast<float*>(wb + L.cov);
  float* y[2] = {reinterpret_cast<float*>(wb + L.y0), reinterpret_cast<float*>(wb + L.y1)};
  float* q = reinterpret_cast<float*>(wb + L.q);
  hipLaunchKernelGGL(k_colmean, dim3(C / 64), dim3(1024), 0, s, x, mask, n, C, mean, count);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_cov, dim3(C / 64, C / 64), dim3(256), 0, s, x, mask, n, C, mean, count, cov);
  DVT_CHECK_LAUNCH();
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(k_pca_iter, dim3(C / 64), dim3(256), 0, s, cov, y[(it + 1) & 1], it == 0 ? 1 : 0, C, y[it & 1], q);
    DVT_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_pca_finish, dim3(1), dim3(256), 0, s, y[(iters - 1) & 1], q, C, count, basis, evals);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_vis_project(const float* x, const float* basis, const float* rgb_min, const float* rgb_max, int n, int C, float* out,
                    void* stream) {
  if (x == nullptr || basis == nullptr || out == nullptr || !shape_ok(n, C) || ((rgb_min == nullptr) != (rgb_max == nullptr)))
    return DVT_E_BADARG;
  hipLaunchKernelGGL(k_rows, dim3(dvt_cdiv(n, 4)), dim3(256), 0, static_cast<hipStream_t>(stream), x, n, C, 0, basis, rgb_min,
                     rgb_max, 0, out);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_vis_robust_range(const float* colors, const uint8_t* mask, int n, float m, float* range, double* stats, int32_t* rows,
                         void* work, int64_t work_bytes, void* stream) {
  if (colors == nullptr || range == nullptr || work == nullptr || n < 1 || n > DVT_VIS_MAX_ROWS || !(m > 0.0f))
    return DVT_E_BADARG;
  const VisLayout L = vis_layout(n, 64, 0, 0);
  if (work_bytes < L.total) return DVT_E_BADARG;
  static_assert(3 * sizeof(RangeRec) <= kScratchBytes, "scratch section too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  RangeRec* rec = reinterpret_cast<RangeRec*>(static_cast<char*>(work) + L.scratch);
  hipLaunchKernelGGL(k_robust, dim3(3), dim3(1024), 0, s, colors, mask, n, m, rec);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_robust_finish, dim3(1), dim3(64), 0, s, rec, range, stats, rows);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_vis_fg_mask(const float* colors, int n, float thresh, uint8_t* mask_out, void* stream) {
  if (colors == nullptr || mask_out == nullptr || n < 1 || n > DVT_VIS_MAX_ROWS) return DVT_E_BADARG;
  hipLaunchKernelGGL(k_fg_mask, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), colors, n, thresh, mask_out);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_vis_norm_map(const float* x, int n, int C, float* out, void* work, int64_t work_bytes, void* stream) {
  if (x == nullptr || out == nullptr || work == nullptr || !shape_ok(n, C)) return DVT_E_BADARG;
  const VisLayout L = vis_layout(n, C, 0, 0);
  if (work_bytes < L.total) return DVT_E_BADARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* tmp = reinterpret_cast<float*>(static_cast<char*>(work) + L.tmp);
  hipLaunchKernelGGL(k_rows, dim3(dvt_cdiv(n, 4)), dim3(256), 0, s, x, n, C, 1, (const float*)nullptr, (const float*)nullptr,
                     (const float*)nullptr, 0, tmp);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_minmax_norm, dim3(1), dim3(1024), 0, s, tmp, n, 1e-6f, -1, out);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_vis_similarity_map(const float* x, int h, int w, int C, float* out, void* work, int64_t work_bytes, void* stream) {
  if (h < 1 || w < 1 || (int64_t)h * w > DVT_VIS_MAX_ROWS) return DVT_E_BADARG;
  const int n = h * w;
  if (x == nullptr || out == nullptr || work == nullptr || !shape_ok(n, C)) return DVT_E_BADARG;
  const VisLayout L = vis_layout(n, C, 0, 0);
  if (work_bytes < L.total) return DVT_E_BADARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* tmp = reinterpret_cast<float*>(static_cast<char*>(work) + L.tmp);
  const int center = (h / 2) * w + w / 2;
  hipLaunchKernelGGL(k_rows, dim3(dvt_cdiv(n, 4)), dim3(256), 0, s, x, n, C, 2, (const float*)nullptr, (const float*)nullptr,
                     (const float*)nullptr, center, tmp);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_minmax_norm, dim3(1), dim3(1024), 0, s, tmp, n, 0.0f, center, out);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_vis_kmeans(const float* x, int n, int C, int K, const int32_t* init_rows, const float* init_centers, int num_init,
                   int max_iter, float tol, int32_t* labels, float* centers, double* inertia, int32_t* iterations,
                   int32_t* best, void* work, int64_t work_bytes, void* stream) {
  if (x == nullptr || labels == nullptr || centers == nullptr || inertia == nullptr || iterations == nullptr ||
      work == nullptr || !shape_ok(n, C) || K < 1 || K > DVT_VIS_MAX_K || K > n || num_init < 1 ||
      num_init > DVT_VIS_MAX_INIT || max_iter < 1 || max_iter > DVT_VIS_MAX_ITER ||
      (init_rows == nullptr && init_centers == nullptr))
    return DVT_E_BADARG;
  const VisLayout L = vis_layout(n, C, K, num_init);
  if (work_bytes < L.total) return DVT_E_BADARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* wb = static_cast<char*>(work);
  KmPtrs p;
  p.centers = reinterpret_cast<float*>(wb + L.km_centers);
  p.cnorm = reinterpret_cast<double*>(wb + L.km_cnorm);
  p.labels = reinterpret_cast<int32_t*>(wb + L.km_labels);
  p.shift = reinterpret_cast<double*>(wb + L.km_shift);
  p.inp = reinterpret_cast<double*>(wb + L.km_inp);
  p.state = reinterpret_cast<int32_t*>(wb + L.km_state);
  p.inertia = reinterpret_cast<double*>(wb + L.km_inertia);
  const int nblk = dvt_cdiv(n, kAssignRows);
  hipLaunchKernelGGL(k_km_init, dim3(K, num_init), dim3(256), 0, s, x, n, C, K, init_rows, init_centers, p);
  DVT_CHECK_LAUNCH();
  for (int it = 0; it < max_iter; ++it) {
    hipLaunchKernelGGL(k_km_control, dim3(num_init), dim3(256), 0, s, it, n, C, K, tol, p);
    DVT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_km_assign, dim3(nblk, num_init), dim3(256), 0, s, x, n, C, K, p);
    DVT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_km_update, dim3(C / 64, num_init), dim3(256), 0, s, x, n, C, K, p);
    DVT_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_km_control, dim3(num_init), dim3(256), 0, s, max_iter, n, C, K, tol, p);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_km_select, dim3(16), dim3(256), 0, s, n, C, K, num_init, p, labels, centers, inertia, iterations, best);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_vis_render_scalar(const float* map, int h, int w, int interp, const float* table, int neg_red, float* canvas,
                          int canvas_h, int canvas_w, int y0, int x0, int H, int W, void* stream) {
  if (map == nullptr || h < 1 || w < 1 || (interp != DVT_VIS_NEAREST && interp != DVT_VIS_BILINEAR) ||
      !rect_ok(canvas, canvas_h, canvas_w, y0, x0, H, W))
    return DVT_E_BADARG;
  const Rect r = {canvas, canvas_h, canvas_w, y0, x0, H, W};
  hipLaunchKernelGGL(k_render_scalar, dim3(dvt_cdiv((int64_t)H * W, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), map,
                     h, w, interp, table, neg_red, r);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_vis_render_rgb(const float* map, int h, int w, int planar, int interp, float* canvas, int canvas_h, int canvas_w,
                       int y0, int x0, int H, int W, void* stream) {
  if (map == nullptr || h < 1 || w < 1 || (interp != DVT_VIS_NEAREST && interp != DVT_VIS_BILINEAR) ||
      !rect_ok(canvas, canvas_h, canvas_w, y0, x0, H, W))
    return DVT_E_BADARG;
  const Rect r = {canvas, canvas_h, canvas_w, y0, x0, H, W};
  hipLaunchKernelGGL(k_render_rgb, dim3(dvt_cdiv((int64_t)H * W, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), map, h,
                     w, planar, interp, r);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_vis_render_labels(const int32_t* labels, int h, int w, const float* table, int K, float* canvas, int canvas_h,
                          int canvas_w, int y0, int x0, int H, int W, void* stream) {
  if (labels == nullptr || table == nullptr || K < 1 || h < 1 || w < 1 || !rect_ok(canvas, canvas_h, canvas_w, y0, x0, H, W))
    return DVT_E_BADARG;
  const Rect r = {canvas, canvas_h, canvas_w, y0, x0, H, W};
  hipLaunchKernelGGL(k_render_labels, dim3(dvt_cdiv((int64_t)H * W, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     labels, h, w, table, K, r);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_vis_fill(float* canvas, int canvas_h, int canvas_w, int y0, int x0, int H, int W, float r, float g, float b,
                 void* stream) {
  if (!rect_ok(canvas, canvas_h, canvas_w, y0, x0, H, W)) return DVT_E_BADARG;
  const Rect rc = {canvas, canvas_h, canvas_w, y0, x0, H, W};
  hipLaunchKernelGGL(k_fill, dim3(dvt_cdiv((int64_t)H * W, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), rc, r, g, b);
  DVT_CHECK_LAUNCH();
  return 0;
}

int dvt_vis_canvas_to_u8(const float* canvas, int canvas_h, int canvas_w, uint8_t* out, void* stream) {
  if (canvas == nullptr || out == nullptr || canvas_h < 1 || canvas_w < 1 || canvas_h > 32768 || canvas_w > 32768)
    return DVT_E_BADARG;
  const int64_t pixels = (int64_t)canvas_h * canvas_w;
  hipLaunchKernelGGL(k_to_u8, dim3(dvt_cdiv(pixels, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), canvas, pixels, out);
  DVT_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
