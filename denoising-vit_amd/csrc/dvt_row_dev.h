// Device helpers of the trainers' row-local kernels (one wave per row of C floats): the row type, float4 arithmetic and the
// one-wave-per-row launch.  Only what a kernel needs at compile time lives here; the kernels that stages 2 and 3 share are
// compiled once, in dvt_block_train.hip.
#pragma once
#include "dvt_common.h"

// ---- a row of C floats held by one wave: float4 index lane + 64 j, j < NJ -------------------------------
template <int C>
struct Row {
  static constexpr int NJ = (C / 4 + 63) / 64;
  float4 v[NJ];
  __device__ __forceinline__ void load(const float* p, int lane) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int i = lane + 64 * j;
      v[j] = (i < C / 4) ? p4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __device__ __forceinline__ void store(float* p, int lane) const {
    float4* p4 = reinterpret_cast<float4*>(p);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int i = lane + 64 * j;
      if (i < C / 4) p4[i] = v[j];
    }
  }
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int j = 0; j < NJ; ++j) v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __device__ __forceinline__ float sum() const {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    return wave_sum(s);
  }
};
#define ROW_FOR(j, NJ) _Pragma("unroll") for (int j = 0; j < NJ; ++j)

__device__ __forceinline__ float4 f4_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 f4_sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 f4_mul(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 f4_scale(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ float f4_dot(float4 a, float4 b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }

// one wave per row, four rows per 256-thread workgroup
template <typename K, typename... A>
int launch_rows(K kernel, int R, hipStream_t s, A... args) {
  hipLaunchKernelGGL(kernel, dim3(dvt_cdiv(R, 4)), dim3(256), 0, s, args...);
  DVT_CHECK_LAUNCH();
  return 0;
}
