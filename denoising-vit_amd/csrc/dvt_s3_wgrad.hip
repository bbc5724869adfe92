// bf16 split-K weight gradient of the stage-3 step's gemm_modes 5 and 7 (include/dvt_stage3.h):
//   dW[n][k] (+)= sum_r bf16(dy[r][n]) * bf16(x[r][k])   v_mfma_f32_32x32x16_bf16, fp32 accumulation
//   db[n]    (+)= sum_r dy[r][n]                          from the UNROUNDED fp32 dy
// R % 128 == n % 128 == k % 128 == 0.  The operands are the row casts of dvt_s3_cast.hip (round to nearest even), bf16 [R][n]
// and [R][k]: nothing is transposed in memory.
//
// s3_wgrad_kernel: tile 128 (n) x 128 (k) per workgroup, 256 threads = 4 waves as 2 x 2, each wave 64 x 64 = 2 x 2 accumulator
//   blocks of 32 x 32.  A row step is 64 token rows of each operand, [64][128] bf16 as they lie in memory (256-byte rows),
//   brought in by LDS-DMA (16 B per lane, four rows per wave instruction) into one of two stages: 2 stages x 2 operands x
//   16 KB = 64 KB of LDS in one object, two workgroups per CU.  Compiler's resource summary of the shipped build: see the
//   table at "Resources" below.
//
//   Both operands have the reduction index r OUTERMOST, an MFMA operand wants 8 consecutive r per lane: the fragments are read
//   with the transposed LDS read ds_read_b64_tr_b16.  Per 16-lane group it takes a block of 4 rows x 16 columns, lane 4 q + p of
//   the group supplying the address of row q, columns 4 p .. 4 p + 3 (8 bytes, 8-byte aligned), and hands lane i column i with
//   row q in element q.  For the 32x32x16 operand (lane l: column l & 31, r = 8 (l >> 5) + j, j < 8) that is two reads per
//   fragment (rows 8 h + 0..3 and 8 h + 4..7 of the 16-row MFMA step), groups 0 / 1 of a 32-lane half taking columns 0..15 /
//   16..31.  Every lane of every wave takes part in every read (no branch around them): EXEC is all ones.
//
//   LDS image and its bank conflicts: plain 256-byte rows, the 16-byte chunk c (0..15) of row r stored at chunk
//   c ^ ((r & 3) << 2).  A 32-lane half of one transposed read covers 4 rows (r & 3 = 0..3) x 64 bytes (4 aligned chunks c0 ..
//   c0 + 3): without the XOR all four rows fall on the same 16 of the 64 banks (bank = (byte / 4) % 64, row pitch 256 B = 64
//   banks), a 4-way conflict; with it row q's chunks land in quarter (c0 / 4) ^ q of the bank row, the 32 lanes x 2 banks cover
//   all 64 banks once: computed conflicts 0.  The DMA writes lane-linearly, so the XOR is applied to the SOURCE chunk of the
//   lane that fills a slot (the same involution on both sides).
//
//   grid (tiles, S): workgroup (t, c) sums chunk c of the R / 64 row steps into the fp32 partial tile part[c][n][k] (plain
//   stores).  s3_wgrad_reduce_kernel then forms dw (+)= part[0] + part[1] + ... (ascending chunk order, then the one add into dw).  No
//   float atomics anywhere: two runs give the same bits.
//
// Split rule (dvt_s3_wgrad_splits; a function of (R, n, k) alone): with steps = R / 64 and tiles = (n / 128) (k / 128),
//   S = min(ceil(1024 / tiles), steps / 4), at least 1
//   -- two rounds of the chip's 512 workgroup slots (256 CUs x 2), never fewer than 4 row steps per chunk.  Chunk c takes
//   steps / S row steps, the first steps % S chunks one more.  ViT-B/14 at 518 x 518, batch 64 (R = 90 112): proj 36 tiles ->
//   S = 29, qkv 108 -> 10, fc1 / fc2 144 -> 8.
//
// s3_colsum_kernel: db from the fp32 dy in a launch of its own.  Rows are cut into Sb = clamp(R / 1024, 1, 128) chunks of
//   whole 128-row blocks; per column and chunk two chains (even rows, odd rows, each ascending) are added to one partial -- the
//   order of the fp32 weight-gradient kernel's column sum (gemm_f32_big_tn_kernel without a split), so that with one chunk the
//   bias gradient has that kernel's bits -- and the reduce kernel adds the partials in ascending chunk order.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage of this file as shipped):
//   kernel                   VGPR  AGPR  SGPR  LDS bytes  occupancy (waves / SIMD)
//   s3_wgrad_kernel            64    64    33      65 536   2 (the LDS admits two workgroups per CU)
//   s3_wgrad_reduce_kernel     18     0    22           0   8
//   s3_colsum_kernel           19     0    22         512   8
#include "dvt_block_train.h"
#include "../../include/dvt_stage3.h"

namespace {

typedef short wg_s4 __attribute__((ext_vector_type(4)));
typedef short wg_s8 __attribute__((ext_vector_type(8)));
typedef float wg_f16 __attribute__((ext_vector_type(16)));

constexpr int WG_T = 128;                       // tile edge, both ways
constexpr int WG_BR = 64;                       // token rows per row step
constexpr int WG_OPER_BYTES = WG_BR * WG_T * 2;  // one operand of one stage: 16 KB
constexpr int WG_STAGE_BYTES = 2 * WG_OPER_BYTES;

__device__ __forceinline__ void wg_glds16(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// 64 rows x 256 bytes of X (bf16, leading dimension ld elements) from (row0, col0) into the image described above
__device__ __forceinline__ void wg_stage(const uint16_t* __restrict__ X, int ld, int64_t row0, int col0, char* lds, int wave, int lane) {
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int slot = it * 256 + wave * 64 + lane;  // 16-byte slot of the image: row slot >> 4, stored chunk slot & 15
    const int row = slot >> 4, chunk = (slot & 15) ^ ((row & 3) << 2);
    wg_glds16(X + (size_t)(row0 + row) * ld + col0 + chunk * 8, lds + (it * 256 + wave * 64) * 16);
  }
}

__device__ __forceinline__ wg_s4 wg_read_tr(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) wg_s4*)p);
}

// the 32x32x16 fragment of columns cb .. cb + 31 (cb % 32 == 0), MFMA step ks (rows 16 ks .. 16 ks + 15) of one operand image;
// `lane_off`: the lane's share of the address, formed once in the kernel
__device__ __forceinline__ wg_s8 wg_frag(const char* img, int lane_off, int q, int cb, int ks) {
  // row of this lane's address: 16 ks + 8 h + 4 t + q, so row & 3 == q; chunk cb / 8 + 2 (group & 1) + (p >> 1), XORed with 4 q
  const char* p = img + ks * 16 * 256 + (((cb >> 3) ^ (q << 2)) << 4) + lane_off;
  const wg_s4 lo = wg_read_tr(p), hi = wg_read_tr(p + 4 * 256);
  return wg_s8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

__global__ __launch_bounds__(256) void s3_wgrad_kernel(const uint16_t* __restrict__ dyb, const uint16_t* __restrict__ xb,
                                                       float* __restrict__ part, int n, int k, int steps, int S) {
  __shared__ __attribute__((aligned(16))) char smem[2 * WG_STAGE_BYTES];  // 64 KB, one LDS object
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int kt = k / WG_T, n0 = (blockIdx.x / kt) * WG_T, k0 = (blockIdx.x % kt) * WG_T;
  const int c = blockIdx.y, base = steps / S, rem = steps % S;
  const int first = c * base + (c < rem ? c : rem), cnt = base + (c < rem ? 1 : 0);
  wg_f16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  // lane 4 q + p of 16-lane group g (h = g >> 1): row 8 h + q of the step, chunk 2 (g & 1) + (p >> 1), byte 8 (p & 1) in it.  The
  // chunk offset 2 (g & 1) + (p >> 1) < 4 only touches the two low chunk bits, the XOR (4 q) only the two above: they add
  const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  const int lane_off = ((g >> 1) * 8 + q) * 256 + ((2 * (g & 1) + (pp >> 1)) << 4) + 8 * (pp & 1);
#define WG_ISSUE(st)                                                                                   \
  do {                                                                                                 \
    char* st_ = smem + ((st) & 1) * WG_STAGE_BYTES;                                                    \
    wg_stage(dyb, n, (int64_t)(first + (st)) * WG_BR, n0, st_, wave, lane);                            \
    wg_stage(xb, k, (int64_t)(first + (st)) * WG_BR, k0, st_ + WG_OPER_BYTES, wave, lane);             \
  } while (0)
  if (cnt > 0) WG_ISSUE(0);
  for (int st = 0; st < cnt; ++st) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (st + 1 < cnt) WG_ISSUE(st + 1);
    const char* A = smem + (st & 1) * WG_STAGE_BYTES;
    const char* B = A + WG_OPER_BYTES;
#pragma unroll
    for (int ks = 0; ks < WG_BR / 16; ++ks) {
      const wg_s8 a0 = wg_frag(A, lane_off, q, wm * 64, ks), a1 = wg_frag(A, lane_off, q, wm * 64 + 32, ks);
      const wg_s8 b0 = wg_frag(B, lane_off, q, wn * 64, ks), b1 = wg_frag(B, lane_off, q, wn * 64 + 32, ks);
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
#undef WG_ISSUE
  // C/D layout of the 32x32 MFMA: col = lane & 31 (k), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (n)
  float* out = part + (size_t)c * n * k;
  const int l31 = lane & 31, kh = lane >> 5;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gn = n0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        out[(size_t)gn * k + k0 + wn * 64 + j * 32 + l31] = acc[i][j][r];
      }
}

// dw[i] = (acc ? dw[i] : 0) + (part[0][i] + ... + part[S - 1][i]) over n4 float4; then the same for db over its nb4 float4 with
// Sb partials (the threads behind n4)
__global__ __launch_bounds__(256) void s3_wgrad_reduce_kernel(const float4* __restrict__ part, float4* __restrict__ dw, int64_t n4,
                                                              int S, const float4* __restrict__ bpart, float4* __restrict__ db,
                                                              int nb4, int Sb, int acc) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4 + nb4) return;
  int64_t stride = n4;
  float4* dst = dw;
  if (i >= n4) {
    i -= n4, part = bpart, dst = db, stride = nb4, S = Sb;
  }
  float4 v = part[i];
  for (int s = 1; s < S; ++s) {
    const float4 p = part[(int64_t)s * stride + i];
    v.x += p.x, v.y += p.y, v.z += p.z, v.w += p.w;
  }
  if (acc) {  // one rounding on top of the overwriting result
    const float4 o = dst[i];
    v.x += o.x, v.y += o.y, v.z += o.z, v.w += o.w;
  }
  dst[i] = v;
}

// bpart[c][col] = (sum of the even rows of chunk c, ascending) + (sum of its odd rows, ascending); grid (n / 128, Sb), thread
// (col = tid & 127, parity = tid >> 7); chunks of whole 128-row blocks
__global__ __launch_bounds__(256) void s3_colsum_kernel(const float* __restrict__ dy, float* __restrict__ bpart, int n, int blocks128,
                                                        int Sb) {
  __shared__ float odd[128];
  const int col = threadIdx.x & 127, par = threadIdx.x >> 7, c = blockIdx.y;
  const int base = blocks128 / Sb, rem = blocks128 % Sb;
  const int64_t first = ((int64_t)c * base + (c < rem ? c : rem)) * 128, rows = (int64_t)(base + (c < rem ? 1 : 0)) * 128;
  const float* src = dy + (size_t)(first + par) * n + blockIdx.x * 128 + col;
  float sum = 0.f;
  for (int64_t r = 0; r < rows; r += 16) {  // rows % 128 == 0
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(r + 2 * u) * n];
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += v[u];
  }
  if (par) odd[col] = sum;
  __syncthreads();
  if (!par) bpart[(size_t)c * n + blockIdx.x * 128 + col] = sum + odd[col];
}

int64_t up256(int64_t b) { return (b + 255) / 256 * 256; }
bool shape_ok(int64_t R, int n, int k) {
  return R >= 128 && R % 128 == 0 && n >= 128 && n % 128 == 0 && k >= 128 && k % 128 == 0 && R <= (int64_t)1 << 30 &&
         (int64_t)(n / WG_T) * (k / WG_T) <= 65535;
}
int colsum_splits(int64_t R) {
  const int64_t s = R / 1024;
  return s < 1 ? 1 : s > 128 ? 128 : (int)s;
}
int resolve_splits(int64_t R, int n, int k, int splits) {
  const int steps = (int)(R / WG_BR);
  if (splits == 0) return dvt_s3_wgrad_splits(R, n, k);
  const int most = steps < 65535 ? steps : 65535;  // (a grid dimension)
  return splits > most ? most : splits;
}

}  // namespace

int dvt_s3_wgrad_splits(int64_t R, int n, int k) {
  const int64_t steps = R / WG_BR, tiles = (int64_t)(n / WG_T) * (k / WG_T);
  int64_t s = (1024 + tiles - 1) / tiles;
  if (s > steps / 4) s = steps / 4;
  return s < 1 ? 1 : (int)s;
}

int64_t dvt_s3_wgrad_partial_bytes(int64_t R, int n, int k, int S) {
  return up256((int64_t)S * n * k * 4) + up256((int64_t)colsum_splits(R) * n * 4);
}

int dvt_s3_wgrad_bf16_run(const uint16_t* dyb, const uint16_t* xb, const float* dy, float* dw, float* db, void* partial, int64_t R,
                          int n, int k, int S, int accumulate, hipStream_t s) {
  const int steps = (int)(R / WG_BR), Sb = colsum_splits(R);
  float* part = reinterpret_cast<float*>(partial);
  float* bpart = reinterpret_cast<float*>(reinterpret_cast<char*>(partial) + up256((int64_t)S * n * k * 4));
  hipLaunchKernelGGL(s3_wgrad_kernel, dim3((n / WG_T) * (k / WG_T), S), dim3(256), 0, s, dyb, xb, part, n, k, steps, S);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(s3_colsum_kernel, dim3(n / 128, Sb), dim3(256), 0, s, dy, bpart, n, (int)(R / 128), Sb);
  DVT_CHECK_LAUNCH();
  const int64_t n4 = (int64_t)n * k / 4;
  hipLaunchKernelGGL(s3_wgrad_reduce_kernel, dim3(dvt_cdiv(n4 + n / 4, 256)), dim3(256), 0, s, (const float4*)part, (float4*)dw, n4, S,
                     (const float4*)bpart, (float4*)db, n / 4, Sb, accumulate);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t dvt_s3_wgrad_bf16_scratch_bytes(int64_t R, int n, int k, int splits) {
  if (!shape_ok(R, n, k) || splits < 0) return -1;
  return up256(R * n * 2) + up256(R * k * 2) + dvt_s3_wgrad_partial_bytes(R, n, k, resolve_splits(R, n, k, splits));
}

extern "C" int dvt_s3_wgrad_bf16(const float* dy, const float* x, float* dw, float* db, void* scratch, int64_t scratch_bytes,
                                 int64_t R, int n, int k, int splits, int accumulate, void* stream) {
  if (!dy || !x || !dw || !db || !scratch || !shape_ok(R, n, k) || splits < 0) return DVT_E_BADARG;
  if (!dvt_aligned16(dy) || !dvt_aligned16(x) || !dvt_aligned16(dw) || !dvt_aligned16(db) || !dvt_aligned16(scratch))
    return DVT_E_BADARG;
  if (scratch_bytes < dvt_s3_wgrad_bf16_scratch_bytes(R, n, k, splits)) return DVT_E_BADARG;
  char* base = reinterpret_cast<char*>(scratch);
  uint16_t* dyb = reinterpret_cast<uint16_t*>(base);
  uint16_t* xb = reinterpret_cast<uint16_t*>(base + up256(R * n * 2));
  DVT_TRY(dvt_s3_cast_bf16(dy, dyb, R, n, stream));
  DVT_TRY(dvt_s3_cast_bf16(x, xb, R, k, stream));
  return dvt_s3_wgrad_bf16_run(dyb, xb, dy, dw, db, base + up256(R * n * 2) + up256(R * k * 2), R, n, k,
                               resolve_splits(R, n, k, splits), accumulate != 0, (hipStream_t)stream);
}
