// What the two linear-probe heads (dvt_seg.hip, dvt_depth.hip) share on the device: the source index of a bilinear
// resize and the two 64 x 64 fp32 tiles of a 1 x 1 convolution -- logits and parameter-gradient slab.  The tiles take
// their element loads as callables, so a head states only where its X and W come from; epilogues stay with the kernels.
#pragma once
#include "dvt_common.h"

namespace {

// Source index of a bilinear resize (PyTorch upsample_bilinear2d, align_corners=False, size given):
//   src = (in / out) (dst + 0.5) - 0.5, clamped below at 0;  i0 = (int) src;  i1 = i0 + (i0 < in - 1);  l1 = src - i0.
struct Src {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ Src src_index(int dst, int in, float scale) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  Src r;
  r.i0 = (int)s;
  r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
  r.l1 = s - (float)r.i0;
  r.l0 = 1.f - r.l1;
  return r;
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Logits tile of a block of 256 threads: acc += X [n0 .. n0 + 64, :C] W [k0 .. k0 + 64, :C]^T, 32 channels per stage;
// thread (ty, tx) = (threadIdx.x >> 4, threadIdx.x & 15) owns rows n0 + 4 ty + i and classes k0 + 4 tx + j.
// load_x(row, c) is called for row < n only, load_w(k, c) for k < K only; the rest of the tile is zero.
template <typename LoadX, typename LoadW>
__device__ __forceinline__ void head_logits_tile(int64_t n0, int64_t n, int k0, int K, int C, LoadX load_x, LoadW load_w,
                                                 float (&acc)[4][4]) {
  __shared__ float xs[32][65];
  __shared__ float as[32][65];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  for (int c0 = 0; c0 < C; c0 += 32) {
    for (int e = threadIdx.x; e < 64 * 32; e += 256) {
      const int r = e >> 5, cc = e & 31;
      const int64_t row = n0 + r;
      xs[cc][r] = row < n ? load_x(row, c0 + cc) : 0.f;
      const int kk = k0 + r;
      as[cc][r] = kk < K ? load_w(kk, c0 + cc) : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int cc = 0; cc < 32; ++cc) {
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = xs[cc][ty * 4 + i];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = as[cc][tx * 4 + j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
}

// Parameter-gradient slab of a block of 256 threads, grid (C / 64, ceil(K / 64), slabs): Gp [slab, K, C] = dZ^T X over
// rows [r0, r1) in stages of 32; blocks of the first channel tile also write dbp [slab, K], the column sums of dZ.
// load_x(row, c) is called for row < r1 only.
template <typename LoadX>
__device__ __forceinline__ void head_pgrad_slab(int64_t r0, int64_t r1, int slab, const float* __restrict__ dz, int C, int K,
                                                LoadX load_x, float* __restrict__ Gp, float* __restrict__ dbp) {
  __shared__ float ds[32][65];
  __shared__ float xs[32][65];
  const int c0 = blockIdx.x * 64, k0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc[4][4] = {};
  float dbacc = 0.f;
  for (int64_t rb = r0; rb < r1; rb += 32) {
    for (int e = threadIdx.x; e < 32 * 64; e += 256) {
      const int r = e >> 6, cc = e & 63;
      const int64_t row = rb + r;
      const int kk = k0 + cc;
      ds[r][cc] = (row < r1 && kk < K) ? dz[row * K + kk] : 0.f;
      xs[r][cc] = row < r1 ? load_x(row, c0 + cc) : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < 32; ++r) {
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = ds[r][ty * 4 + i];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = xs[r][tx * 4 + j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
    if (blockIdx.x == 0 && threadIdx.x < 64)
      for (int r = 0; r < 32; ++r) dbacc += ds[r][threadIdx.x];
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int kk = k0 + ty * 4 + i;
    if (kk >= K) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) Gp[((size_t)slab * K + kk) * C + c0 + tx * 4 + j] = acc[i][j];
  }
  if (blockIdx.x == 0 && threadIdx.x < 64 && k0 + (int)threadIdx.x < K) dbp[(size_t)slab * K + k0 + threadIdx.x] = dbacc;
}

}  // namespace
