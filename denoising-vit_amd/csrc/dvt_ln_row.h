// The row-local LayerNorm arithmetic of the ViT extractor, one wave per row: shared by layernorm_kernel (dvt_vit.hip),
// layernorm_f32_kernel (dvt_vit_f32.hip) and the tap kernel, so that a tapped layer carries the bits of the final-norm launch.
#pragma once
#include <hip/hip_runtime.h>

#include "dvt_common.h"

// Load the row (nq = dim / 4 float4 pieces, lane + 64 i in slot i; NV slots: 4 up to dim 1024, 6 up to 1536) and reduce its
// (mean, rstd) in two passes over the registers.
template <int NV>
__device__ __forceinline__ void ln_row_stats(const float4* __restrict__ xr, int nq, int dim, float eps, int lane,
                                             float4 (&v)[NV], float& mean, float& rstd) {
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int q = lane + 64 * i;
    if (q < nq) {
      v[i] = xr[q];
      sum += v[i].x + v[i].y + v[i].z + v[i].w;
    }
  }
  mean = wave_sum(sum) / (float)dim;
  float var = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int q = lane + 64 * i;
    if (q < nq) {
      const float a = v[i].x - mean, bq = v[i].y - mean, cq = v[i].z - mean, d = v[i].w - mean;
      var += a * a + bq * bq + cq * cq + d * d;
    }
  }
  rstd = rsqrtf(wave_sum(var) / (float)dim + eps);
}

// One float4 piece of the normalised row: (v - mean) * rstd * w + b
__device__ __forceinline__ float4 ln_row_piece(const float4 v, float mean, float rstd, const float4 ww, const float4 bb) {
  return make_float4((v.x - mean) * rstd * ww.x + bb.x, (v.y - mean) * rstd * ww.y + bb.y,
                     (v.z - mean) * rstd * ww.z + bb.z, (v.w - mean) * rstd * ww.w + bb.w);
}
