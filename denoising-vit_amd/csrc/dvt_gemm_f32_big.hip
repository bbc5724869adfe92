// Exact-fp32 GEMM on the 128 x 128 x 32 tile: the forward layers of the fp32 extractor (dvt_vit_f32.hip, with its fused GELU /
// residual epilogues) and the forward, data-gradient and weight-gradient products of stages 2 / 3 (dvt_block_train.hip).
// Shapes the tile does not take go to the LDS-DMA ring (dvt_gemm_f32_glds.hip) or to the register-staged kernel
// (dvt_gemm_f32.hip), through their launchers.
#include "dvt_gemm_f32_dev.h"
#include "dvt_tune.h"

namespace {

// ---- 128 x 128 x 32 tile for LARGE-m forward layers (the fp32 extractor: m = views x 1408 tokens) ----------------------
// Round 5 ("fp32 extractor GEMM 109 -> >= 125 TF/s").  The 64 x 64 tiles give every wave ONE 32 x 32
// accumulator: per MFMA (64 cycles) a wave reads two fragment values per lane from LDS and a workgroup moves (64 + 64) rows
// through L2 -> LDS per 64 x 64 outputs.  Here a wave owns 64 x 64 outputs = 2 x 2 accumulators (64 VGPRs): every A / B
// fragment value feeds TWO MFMAs, four independent 64-cycle accumulation chains keep the pipe issuing back to back, and the
// workgroup's operand traffic per flop halves.  BK = 32 keeps the LDS rows at 128 B (whole lines per DMA row piece), the
// stage at 32 KB and TWO stages at 64 KB, i.e. TWO workgroups per CU (one wave each per SIMD) that fill each other's
// barrier / fragment-read gaps, as in the 64 x 64 ring.  LDS image: lane-linear rows of 32 floats, 16-B chunk c of row r at
// position c ^ ((r >> 1) & 7) (applied at the DMA source and at the b128 fragment reads: the 16 lanes of a read group cover
// all 64 banks).  Both operands k-contiguous, M % 128 == N % 128 == K % 32 == 0 (the caller falls back otherwise).
constexpr int GB_BK = 32;
constexpr int GB_TILE_FLOATS = 128 * GB_BK;        // one operand tile: 16 KB
constexpr int GB_STAGE_FLOATS = 2 * GB_TILE_FLOATS;  // A + B: 32 KB

__device__ __forceinline__ void stage_big(const float* __restrict__ X, int ld, int r0, int k0, float* lds, int wave, int lane) {
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int s = it * 256 + wave * 64 + lane;  // 16-B slot of the 16-KB tile: row s >> 3, position s & 7
    const int row = s >> 3, c = (s & 7) ^ ((row >> 1) & 7);
    glds16f(X + (size_t)(r0 + row) * ld + k0 + c * 4, lds + (it * 256 + wave * 64) * 4);
  }
}

// 16-B piece q (k-values 4 q .. 4 q + 3 of k half `kh`) of row `row`: what one lane feeds into MFMA steps 4 q .. 4 q + 3
__device__ __forceinline__ float4 frag4_big(const float* __restrict__ S, int row, int kh, int q) {
  return *reinterpret_cast<const float4*>(S + row * GB_BK + (((kh * (GB_BK / 8) + q) ^ ((row >> 1) & 7)) << 2));
}

template <int EPI>
__global__ __launch_bounds__(256) void gemm_f32_big_kernel(GemmArgs p) {
  __shared__ __attribute__((aligned(16))) float smem[2 * GB_STAGE_FLOATS];  // 64 KB, one LDS object
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int n0 = blockIdx.x * 128, m0 = blockIdx.y * 128;
  const int nk = p.K / GB_BK;
  floatx16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
#define GB_ISSUE(kt)                                                             \
  do {                                                                           \
    float* st_ = smem + ((kt) & 1) * GB_STAGE_FLOATS;                            \
    stage_big(p.A, p.lda, m0, (kt) * GB_BK, st_, wave, lane);                    \
    stage_big(p.B, p.ldb, n0, (kt) * GB_BK, st_ + GB_TILE_FLOATS, wave, lane);   \
  } while (0)
  GB_ISSUE(0);
  const int l31 = lane & 31, kh = lane >> 5;
  for (int kt = 0; kt < nk; ++kt) {
    // tile kt has landed (own DMAs), everyone's has, and everyone is done reading the other buffer (tile kt - 1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 1 < nk) GB_ISSUE(kt + 1);
    const float* As = smem + (kt & 1) * GB_STAGE_FLOATS;
    const float* Bs = As + GB_TILE_FLOATS;
    // reads in the order the MFMA steps need them (piece q of all four fragments, then q + 1): the first 16 MFMAs can
    // start behind four reads instead of thirteen
    float4 fa[2][GB_BK / 8], fb[2][GB_BK / 8];
#pragma unroll
    for (int q = 0; q < GB_BK / 8; ++q)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[i][q] = frag4_big(As, wm * 64 + i * 32 + l31, kh, q);
        fb[i][q] = frag4_big(Bs, wn * 64 + i * 32 + l31, kh, q);
      }
#pragma unroll
    for (int q = 0; q < GB_BK / 8; ++q) {
#define GB_STEP(E)                                                                                          \
  _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                             \
  _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                             \
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][q].E, fb[j][q].E, acc[i][j], 0, 0, 0);
      GB_STEP(x) GB_STEP(y) GB_STEP(z) GB_STEP(w)
#undef GB_STEP
    }
  }
#undef GB_ISSUE
  // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5): a half-wave stores one
  // 128-B row piece per instruction
  // EPI (round 5, the fp32 extractor): the exact-erf GELU of fc1 and the LayerScale + residual of proj / fc2 happen HERE, on
  // the accumulators, instead of in a separate pass that re-read and re-wrote the fp32 [tokens, 3072] / [tokens, 768] tensors
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int gn = n0 + wn * 64 + j * 32 + l31;
    const float bias = p.bias != nullptr ? p.bias[gn] : 0.f;
    const float gm_n = EPI == 2 ? p.gamma[gn] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gm = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        float v = acc[i][j][r] + bias;
        float* c = p.C + (size_t)gm * p.ldc + gn;
        if constexpr (EPI == 1) {
          v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));  // nn.GELU(): exact erf form (as gelu_f32_kernel)
        } else if constexpr (EPI == 2) {
          v = *c + gm_n * v;  // (as resid_f32_kernel: o += g * v)
        } else {
          if (p.relu) v = fmaxf(v, 0.f);
        }
        *c = v;
      }
  }
}

// ---- the same 128 x 128 tile for the WEIGHT-GRADIENT product of the stage-2 trainer (round 6): C[M][N] (+)= sum_k A(m, k) B(k, n) with
// BOTH operands stored reduction-index-major -- A_mem[k][m] = dy[row][out feature], B_mem[k][n] = x[row][in feature]; the
// reduction runs over the 45 056 token rows of a batch, split over blockIdx.z with one atomic add per split and element.
// A stage is 32 rows of each operand, [row][128] floats as they lie in memory (whole 512-B row pieces per LDS-DMA
// instruction, lane-linear: no swizzle needed -- an MFMA 32x32x2 operand is ONE float per lane, lane i of a half-wave reads
// column i of row 2 s + (lane >> 5): 32 consecutive dwords, conflict-free ds_read_b32).  Per stage and wave 64 reads feed 64
// MFMAs (2 x 2 accumulator blocks, four independent chains).  colsum[m] += sum_k A(m, k) (the bias gradient) by the n-tile-0
// blocks from the fragments they read anyway.  Two 32-KB stages = two workgroups per CU, as the forward kernel.
__device__ __forceinline__ void stage_rows_big(const float* __restrict__ X, int ld, int k0, int c0, float* lds, int wave, int lane) {
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int s = it * 256 + wave * 64 + lane;  // 16-B slot: row s >> 5, columns 4 (s & 31) ..
    glds16f(X + (size_t)(k0 + (s >> 5)) * ld + c0 + (s & 31) * 4, lds + (it * 256 + wave * 64) * 4);
  }
}

__global__ __launch_bounds__(256) void gemm_f32_big_tn_kernel(GemmArgs p) {
  __shared__ __attribute__((aligned(16))) float smem[2 * GB_STAGE_FLOATS];  // 64 KB, one LDS object
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int n0 = blockIdx.x * 128, m0 = blockIdx.y * 128;
  const int kbeg = blockIdx.z * p.kchunk, kend = kbeg + p.kchunk < p.K ? kbeg + p.kchunk : p.K;
  const int nk = (kend - kbeg) / GB_BK;
  const bool do_colsum = p.colsum != nullptr && blockIdx.x == 0 && wn == 0;
  floatx16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  float csum[2] = {0.f, 0.f};
#define GT_ISSUE(kt)                                                                       \
  do {                                                                                     \
    float* st_ = smem + ((kt) & 1) * GB_STAGE_FLOATS;                                      \
    stage_rows_big(p.A, p.lda, kbeg + (kt) * GB_BK, m0, st_, wave, lane);                  \
    stage_rows_big(p.B, p.ldb, kbeg + (kt) * GB_BK, n0, st_ + GB_TILE_FLOATS, wave, lane); \
  } while (0)
  if (nk > 0) GT_ISSUE(0);
  const int l31 = lane & 31, kh = lane >> 5;
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 1 < nk) GT_ISSUE(kt + 1);
    const float* As = smem + (kt & 1) * GB_STAGE_FLOATS + kh * 128 + wm * 64 + l31;
    const float* Bs = smem + (kt & 1) * GB_STAGE_FLOATS + GB_TILE_FLOATS + kh * 128 + wn * 64 + l31;
#pragma unroll
    for (int s = 0; s < GB_BK / 2; ++s) {  // rows 2 s + kh of the stage
      const float a0 = As[s * 256], a1 = As[s * 256 + 32], b0 = Bs[s * 256], b1 = Bs[s * 256 + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      if (do_colsum) {
        csum[0] += a0;
        csum[1] += a1;
      }
    }
  }
#undef GT_ISSUE
  // C/D layout of the 32x32 MFMA: col = lane & 31 (n), row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (m)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int gn = n0 + wn * 64 + j * 32 + l31;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gm = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        float* c = p.C + (size_t)gm * p.ldc + gn;
        if (p.atomic)
          atomic_add_f32(c, acc[i][j][r]);
        else
          *c = acc[i][j][r];
      }
  }
  if (do_colsum) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float v = csum[i] + __shfl_xor(csum[i], 32, 64);
      if (kh == 0) atomic_add_f32(p.colsum + m0 + wm * 64 + i * 32 + l31, v);
    }
  }
}

int g_f32_big = 1;  // dvt_tune_set(4, 10 / 11): the 128 x 128 kernels off / on (A/B; results differ in summation order only)

}  // namespace

// This unit's share of dvt_tune_set: two values of key 4 (the rest of that key: dvt_gemm_f32_glds.hip)
int gemm_f32_big_tune(int key, int value) {
  if (key != 4 || (value != 10 && value != 11)) return DVT_TUNE_NOT_MINE;
  g_f32_big = value == 11;  // 11 (default) / 10: dvt_linear_fwd_big takes the 64 x 64 x 64 ring instead
  return 0;
}

// the 128 x 128 x 32 kernel takes this shape (and with it the fused GELU / residual epilogues below)
bool dvt_linear_big_ok(int m, int n, int k) { return g_f32_big && m > 0 && m % 128 == 0 && n % 128 == 0 && k % GB_BK == 0; }

// dw[n][k] (+)= sum_r dy[r][n] x[r][k], db[n] += sum_r dy[r][n] on the 128 x 128 tile (gemm_f32_big_tn_kernel); n, k multiples of
// 128, rows of 32; `accumulate`: atomic adds into dw (the reduction is split so that ~1024 workgroups exist), else ONE split
bool dvt_linear_wgrad_big_ok(int rows, int n, int k) { return g_f32_big && rows > 0 && rows % GB_BK == 0 && n % 128 == 0 && k % 128 == 0; }
int dvt_linear_wgrad_big(const float* dy, const float* x, float* dw, float* db, int rows, int n, int k, int accumulate,
                         hipStream_t s) {
  if (!dy || !x || !dw || !dvt_linear_wgrad_big_ok(rows, n, k)) return DVT_E_BADARG;
  GemmArgs a{};
  a.A = dy; a.B = x; a.C = dw;
  a.M = n; a.N = k; a.K = rows;
  a.lda = n; a.ldb = k; a.ldc = k;
  a.colsum = db;
  a.atomic = accumulate;
  const int tiles = (n / 128) * (k / 128), ktiles = rows / GB_BK;
  int splits = 1;
  if (accumulate) {
    splits = dvt_cdiv(1024, tiles);
    if (splits > ktiles / 8) splits = ktiles / 8;
    if (splits < 1) splits = 1;
  }
  a.kchunk = dvt_cdiv(ktiles, splits) * GB_BK;
  splits = dvt_cdiv(rows, a.kchunk);
  DvtProbeScope probe(DVT_PROBE_FIT_GEMM, s, 2.0 * a.M * a.N * a.K);
  hipLaunchKernelGGL(gemm_f32_big_tn_kernel, dim3(k / 128, n / 128, splits), dim3(256), 0, s, a);
  DVT_CHECK_LAUNCH();
  return 0;
}

// y = epi(x . w^T + b) on the 128 x 128 x 32 kernel ONLY (dvt_linear_big_ok): epi 1 = exact-erf GELU, epi 2 = y += gamma (.) (.)
int dvt_linear_fwd_big_epi(const float* x, const float* w, const float* b, float* y, int m, int n, int k, int epi,
                           const float* gamma, hipStream_t s) {
  if (!x || !w || !y || !dvt_linear_big_ok(m, n, k) || (epi != 1 && epi != 2) || (epi == 2 && !gamma)) return DVT_E_BADARG;
  GemmArgs a = make_fwd(x, w, b, y, m, n, k, 0);
  a.epi = epi;
  a.gamma = gamma;
  DvtProbeScope probe(DVT_PROBE_FIT_GEMM, s, 2.0 * a.M * a.N * a.K);
  if (epi == 1) hipLaunchKernelGGL(gemm_f32_big_kernel<1>, dim3(a.N / 128, a.M / 128), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(gemm_f32_big_kernel<2>, dim3(a.N / 128, a.M / 128), dim3(256), 0, s, a);
  DVT_CHECK_LAUNCH();
  return 0;
}

// Forward linear for LARGE m (the fp32 extractor: m = views x 1408 tokens): the 128 x 128 x 32 kernel where the shape is
// eligible, else the 64 x 64 LDS-DMA ring, whatever the co-residency knob of the fit says.
int dvt_linear_fwd_big(const float* x, const float* w, const float* b, float* y, int m, int n, int k, hipStream_t s) {
  if (!x || !w || !y || m <= 0 || n <= 0 || k <= 0 || (k & 3) || (n & 3)) return DVT_E_BADARG;
  const GemmArgs a = make_fwd(x, w, b, y, m, n, k, 0);
  if (dvt_linear_big_ok(m, n, k)) {
    DvtProbeScope probe(DVT_PROBE_FIT_GEMM, s, 2.0 * a.M * a.N * a.K);
    hipLaunchKernelGGL(gemm_f32_big_kernel<0>, dim3(a.N / 128, a.M / 128), dim3(256), 0, s, a);
    DVT_CHECK_LAUNCH();
    return 0;
  }
  // The ring at the depth of dvt_tune_set(4, 2 / 3).  2 LDS stages (64 KB, the default): two workgroups share a CU and fill
  // each other's barrier / fragment-read gaps -- the stage-2 trainer measured 81 -> 97 TF/s with it; round 3 gave
  // the fp32 extractor the same ring.  Same arithmetic order at either depth: results are bit-identical.
  if ((a.K % BK) == 0 && (a.kchunk % BK) == 0) return gemm_f32_glds_launch(a, 0, 0, 1, s);
  return gemm_f32_staged_fwd(a, s);
}

// ---- component entry point for tests (include/dvt_parts.h): a forwarder only, no kernel and no launch of its own ----
#include "../../include/dvt_parts.h"

extern "C" int dvt_parts_linear_big_epi(const float* x, const float* w, const float* b, float* y, int m, int n, int k, int epi,
                                        const float* gamma, void* stream) {
  if (epi < 0 || epi > 2) return DVT_E_BADARG;
  if (epi == 0) return dvt_linear_fwd_big(x, w, b, y, m, n, k, (hipStream_t)stream);
  return dvt_linear_fwd_big_epi(x, w, b, y, m, n, k, epi, gamma, (hipStream_t)stream);
}
