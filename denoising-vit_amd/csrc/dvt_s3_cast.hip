// fp32 -> bf16 casts of the stage-3 step's mixed-precision mode (include/dvt_stage3.h, gemm_mode 1): the operands of the
// forward and data-gradient GEMMs of qkv / proj / fc1 / fc2 are rounded to bf16 here, immediately before the bf16 GEMM of
// dvt_vit_gemm.hip reads them.  Nothing else of the step is rounded.
//
// Rounding is round-to-nearest-even on the bit pattern (what torch's .to(torch.bfloat16) does): ties go to the even
// mantissa, fp32 denormals become bf16 denormals (the two formats share the exponent range), +-0 keep their sign, a finite
// value above the largest bf16 rounds to infinity, a NaN stays a quiet NaN.  Integer arithmetic, so the result does not depend
// on the wave's denormal mode.
#include "dvt_common.h"
#include "../../include/dvt_stage3.h"

namespace {

__device__ __forceinline__ uint32_t s3_bf16_bits(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;  // NaN
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ uint32_t s3_bf16_pair(float lo, float hi) { return s3_bf16_bits(lo) | (s3_bf16_bits(hi) << 16); }

// y[i] = bf16(x[i]), four elements per thread and trip: one 16-byte load, one 8-byte store; grid-stride
__global__ __launch_bounds__(256) void s3_cast_bf16_kernel(const float4* __restrict__ x, uint2* __restrict__ y, int64_t n4) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const float4 v = x[i];
    y[i] = make_uint2(s3_bf16_pair(v.x, v.y), s3_bf16_pair(v.z, v.w));
  }
}

// wt[k][n] = bf16(w[n][k]), n and k multiples of 64: one 64 x 64 tile per workgroup through LDS.  Both sides move whole row
// pieces: 16 lanes read one 256-byte piece of a row of w (float4 each), 16 lanes write one 128-byte piece of a row of wt
// (four bf16 each).  The tile's pitch of 65 floats leaves the column reads of the second half a 2-way bank conflict
// (ds_read_b32: 32 banks per 32-lane group, rows 4 n4 + j and 4 (n4 + 8) + j) instead of the 16-way one of a pitch of 64.
constexpr int CT = 64, CT_LD = CT + 1;
__global__ __launch_bounds__(256) void s3_cast_bf16_t_kernel(const float* __restrict__ w, uint2* __restrict__ wt, int n, int k) {
  __shared__ float tile[CT][CT_LD];
  const int k0 = blockIdx.x * CT, n0 = blockIdx.y * CT, c = threadIdx.x & 15, r = threadIdx.x >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = r + 16 * i;
    const float4 v = *reinterpret_cast<const float4*>(w + (size_t)(n0 + row) * k + k0 + 4 * c);
    tile[row][4 * c + 0] = v.x;
    tile[row][4 * c + 1] = v.y;
    tile[row][4 * c + 2] = v.z;
    tile[row][4 * c + 3] = v.w;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int kk = r + 16 * i;
    const uint2 o = make_uint2(s3_bf16_pair(tile[4 * c + 0][kk], tile[4 * c + 1][kk]),
                               s3_bf16_pair(tile[4 * c + 2][kk], tile[4 * c + 3][kk]));
    wt[((size_t)(k0 + kk) * n + n0) / 4 + c] = o;
  }
}

}  // namespace

extern "C" int dvt_s3_cast_bf16(const float* x, void* y, int64_t rows, int n, void* stream) {
  if (!x || !y || rows < 1 || n < 4 || n % 4 || !dvt_aligned16(x) || !dvt_aligned16(y)) return DVT_E_BADARG;
  const int64_t n4 = rows * n / 4;
  const int64_t blocks = (n4 + 255) / 256;
  // grid-stride over at most 8 workgroups per CU of the chip's 256
  hipLaunchKernelGGL(s3_cast_bf16_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream,
                     (const float4*)x, (uint2*)y, n4);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int dvt_s3_cast_bf16_t(const float* w, void* wt, int n, int k, void* stream) {
  if (!w || !wt || n < CT || k < CT || n % CT || k % CT || k / CT > 65535 || n / CT > 65535 || !dvt_aligned16(w) || !dvt_aligned16(wt))
    return DVT_E_BADARG;
  hipLaunchKernelGGL(s3_cast_bf16_t_kernel, dim3(k / CT, n / CT), dim3(256), 0, (hipStream_t)stream, w, (uint2*)wt, n, k);
  DVT_CHECK_LAUNCH();
  return 0;
}
