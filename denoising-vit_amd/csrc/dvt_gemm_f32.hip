// Exact-fp32 linear layers of the stage-1 fit on the f32-input matrix cores of gfx950
// (v_mfma_f32_32x32x2_f32: 64 FLOP/clk/SIMD, bitwise an fmaf chain): the register-staged tile family.
//
// Replaces the cuBLAS SGEMMs behind `nn.Sequential(Linear, ReLU, Linear)` of the field MLP
// (dvt/models/neural_feature_field.py:40-44, :49) and of the residual predictor
// (dvt/models/offline_denoiser.py:40-46, :107), forward and backward.
//
// One kernel template covers the three contractions of a linear layer (dvt_gemm_f32_dev.h: operand layouts, Tile and
// gemm_f32_body).  Tile 64x64xBK per 256-thread workgroup (4 waves, each one 32x32 accumulator = 16 VGPRs).
// The small batch (2048 rows) yields few tiles, so wgrad splits the batch reduction over
// blockIdx.z and accumulates with fp32 atomics into a gradient buffer that the fused Adam
// kernel clears (dvt_adam.hip).
// The LDS-DMA ring (dvt_gemm_f32_glds.hip) and the 128 x 128 tile (dvt_gemm_f32_big.hip) are units of their own.
#include "dvt_gemm_f32_dev.h"
#include "dvt_tune.h"

namespace {

template <bool A_KC, bool B_KC, int WM, int WN, int BK>
__global__ __launch_bounds__(64 * WM * WN) void gemm_f32_kernel(GemmArgs p) {
  constexpr int NT = 64 * WM * WN;
  __shared__ __attribute__((aligned(16))) float As[Tile<A_KC, 32 * WM, NT, BK>::LDS_FLOATS];
  __shared__ __attribute__((aligned(16))) float Bs[Tile<B_KC, 32 * WN, NT, BK>::LDS_FLOATS];
  gemm_f32_body<A_KC, B_KC, WM, WN, BK>(p, blockIdx.x, blockIdx.y, blockIdx.z, As, Bs);
}

// ---- grouped launch: up to 4 independent GEMMs in ONE grid -------------------------------------
// At M = 2048 every GEMM of the fit fills only 96-430 workgroups and carries ~4.5 us of fixed
// dependent-latency cost; kernels on different HIP streams did not overlap (measured: wgrad2 ||
// dgrad2 on two streams = 59.8 us, the same as back to back).  Independent GEMMs of one step
// (wgrad + dgrad of a layer, field branch + residual branch) are therefore packed into one
// launch: a workgroup finds its problem from blockIdx.x, the operand layouts become a run-time
// switch over the three instantiations of the same body.
constexpr int MULTI_MAX = 16;  // 4 problems of one fit x DVT_FIT_BATCH_MAX fits
struct MultiArgs {
  int n;
  int blk0[MULTI_MAX + 1];  // first block of each problem
  int gx[MULTI_MAX], gy[MULTI_MAX];
  int layout[MULTI_MAX];  // 0: A k-contig, B k-contig; 1: A k-contig, B row-contig; 2: both row-contig
  GemmArgs g[MULTI_MAX];
};

template <int BK>
__global__ __launch_bounds__(256) void gemm_f32_multi_kernel(MultiArgs m) {
  __shared__ __attribute__((aligned(16))) float As[64 * (BK + 4)];  // >= BK * 64
  __shared__ __attribute__((aligned(16))) float Bs[64 * (BK + 4)];
  int i = 0;
#pragma unroll
  for (int j = 1; j < MULTI_MAX; ++j)
    if (j < m.n && (int)blockIdx.x >= m.blk0[j]) i = j;
  const int local = (int)blockIdx.x - m.blk0[i];
  const int bx = local % m.gx[i], by = (local / m.gx[i]) % m.gy[i], bz = local / (m.gx[i] * m.gy[i]);
  switch (m.layout[i]) {
    case 0: gemm_f32_body<true, true, 2, 2, BK>(m.g[i], bx, by, bz, As, Bs); break;
    case 1: gemm_f32_body<true, false, 2, 2, BK>(m.g[i], bx, by, bz, As, Bs); break;
    default: gemm_f32_body<false, false, 2, 2, BK>(m.g[i], bx, by, bz, As, Bs); break;
  }
}

// ==========================================================================================
// bf16-operand variant of the grouped body (DvtFitConfig.mlp_bf16, the reference's
// `--dtype bfloat16` autocast mode: nn.Linear runs on bf16 casts of fp32 master weights and
// activations; main_img_denoising.py:78).  Operands stay fp32 in HBM and are rounded to bf16
// (RNE, v_cvt_pk_bf16_f32) while they are staged into LDS; accumulation, bias, ReLU, masks and
// every output stay fp32 -- i.e. at least the reference's precision (autocast additionally rounds
// each layer output to bf16).  The fp32-operand body is MFMA-rate bound: one
// v_mfma_f32_32x32x2_f32 (64 cycles) per 2 k per wave, a K = 768 contraction is a dependent chain
// of 24.6 k cycles, ~10 us, whatever the tile/BK/staging (measured).  v_mfma_f32_32x32x16_bf16
// covers 16 k in 32 cycles: the same chain is 1.5 k cycles.
// 64 x 64 tile, 2 x 2 waves, BK = 32 (64 selectable).  LDS rows are k-contiguous bf16, pitch BK + 8
// (conflict-free ds_read_b128 of a lane's 8 k); row-contiguous sources (k slow) are transposed on
// the way in: a thread loads (k, k+1) for 4 rows and writes four packed bf16x2 words.
// ==========================================================================================
typedef short bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 hwbf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
  const hwbf16x2_t v = __builtin_convertvector((f32x2_t){a, b}, hwbf16x2_t);
  return __builtin_bit_cast(uint32_t, v);
}


template <bool KCONTIG, int HBK>
struct TileH {
  static constexpr int HP = HBK + 8;        // bf16 elements per LDS row
  static constexpr int ITERS = HBK / 16;    // float4 per thread per operand tile (256 threads)
  __device__ static __forceinline__ void load(const float* __restrict__ X, int ld, int r0, int Rmax,
                                              int k0, int kend, int tid, float4 regs[ITERS]) {
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (KCONTIG) {
        const int f = tid + 256 * i, r = f / (HBK / 4), kq = f % (HBK / 4);
        const int gr = r0 + r, gk = k0 + 4 * kq;
        if (gr < Rmax && gk < kend) v = *reinterpret_cast<const float4*>(X + (size_t)gr * ld + gk);
      } else {  // regs[2 * it + par] = rows 4*rq .. +3 at k = 2 * (kp + 16 * it) + par
        const int kp = (tid >> 4) + 16 * (i >> 1), rq = tid & 15;
        const int gk = k0 + 2 * kp + (i & 1), gr = r0 + 4 * rq;
        if (gk < kend && gr < Rmax) v = *reinterpret_cast<const float4*>(X + (size_t)gk * ld + gr);
      }
      regs[i] = v;
    }
  }
  __device__ static __forceinline__ void store(uint16_t* __restrict__ S, int tid, const float4 regs[ITERS]) {
    if (KCONTIG) {
#pragma unroll
      for (int i = 0; i < ITERS; ++i) {
        const int f = tid + 256 * i, r = f / (HBK / 4), kq = f % (HBK / 4);
        uint2 w;
        w.x = pack_bf16x2(regs[i].x, regs[i].y);
        w.y = pack_bf16x2(regs[i].z, regs[i].w);
        *reinterpret_cast<uint2*>(S + r * HP + 4 * kq) = w;
      }
    } else {
      const int rq = tid & 15;
      uint32_t* S32 = reinterpret_cast<uint32_t*>(S);
#pragma unroll
      for (int it = 0; it < ITERS / 2; ++it) {
        const int kp = (tid >> 4) + 16 * it;
        const float4 lo = regs[2 * it], hi = regs[2 * it + 1];
        S32[((4 * rq + 0) * HP >> 1) + kp] = pack_bf16x2(lo.x, hi.x);
        S32[((4 * rq + 1) * HP >> 1) + kp] = pack_bf16x2(lo.y, hi.y);
        S32[((4 * rq + 2) * HP >> 1) + kp] = pack_bf16x2(lo.z, hi.z);
        S32[((4 * rq + 3) * HP >> 1) + kp] = pack_bf16x2(lo.w, hi.w);
      }
    }
  }
};

template <bool A_KC, bool B_KC, int HBK>
__device__ __forceinline__ void gemm_bf16op_body(const GemmArgs& p, int bx, int by, int bz,
                                                 uint16_t* __restrict__ As, uint16_t* __restrict__ Bs) {
  using TA = TileH<A_KC, HBK>;
  using TB = TileH<B_KC, HBK>;
  constexpr int HP = TA::HP, NR = TA::ITERS;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int n0 = bx * 64, m0 = by * 64;
  const int kbeg = bz * p.kchunk;
  const int kend = min(p.K, kbeg + p.kchunk);
  if (kbeg >= kend) return;

  floatx16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float csum = 0.f;
  const bool do_colsum = (!A_KC) && p.colsum != nullptr && bx == 0;

  // Cycle stamps of one workgroup (K = 384 .. 768): ~2000 cycles from a tile's global loads to its
  // MFMAs, i.e. with one tile in flight every k-step costs a full memory latency (0.85 us x 6-12
  // steps), and another ~2500 cycles of the epilogue went to the bias / mask loads.  Hence TWO
  // tiles in flight (register sets r0 / r1) and the epilogue operands requested up front.
  float4 ra0[NR], rb0[NR], ra1[NR], rb1[NR];
  TA::load(p.A, p.lda, m0, p.M, kbeg, kend, tid, ra0);
  TB::load(p.B, p.ldb, n0, p.N, kbeg, kend, tid, rb0);
  TA::load(p.A, p.lda, m0, p.M, kbeg + HBK, kend, tid, ra1);  // past kend: zeros, no memory access
  TB::load(p.B, p.ldb, n0, p.N, kbeg + HBK, kend, tid, rb1);
  // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
  const int gn = n0 + wn * 32 + (lane & 31);
  const float bias = (p.bias != nullptr && gn < p.N) ? p.bias[gn] : 0.f;
  float mk[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int gm = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    mk[r] = (p.mask != nullptr && gm < p.M && gn < p.N) ? p.mask[(size_t)gm * p.ldmask + gn] : 1.f;
  }
  // fragment addresses: MFMA step s of a tile uses k = kh * (HBK / 2) + s * 8 + j (j = 0..7, kh = lane >> 5)
  const int kh = lane >> 5;
  const uint16_t* pa = As + (wm * 32 + (lane & 31)) * HP + kh * (HBK / 2);
  const uint16_t* pb = Bs + (wn * 32 + (lane & 31)) * HP + kh * (HBK / 2);
#define H_STEP(RA, RB, KNEXT)                                                                  \
  do {                                                                                         \
    TA::store(As, tid, RA);                                                                    \
    TB::store(Bs, tid, RB);                                                                    \
    __syncthreads();                                                                           \
    TA::load(p.A, p.lda, m0, p.M, (KNEXT), kend, tid, RA); /* two tiles ahead */               \
    TB::load(p.B, p.ldb, n0, p.N, (KNEXT), kend, tid, RB);                                     \
    bf16x8_t fa[HBK / 16], fb[HBK / 16];                                                       \
    _Pragma("unroll") for (int q = 0; q < HBK / 16; ++q) {                                     \
      fa[q] = *reinterpret_cast<const bf16x8_t*>(pa + 8 * q);                                  \
      fb[q] = *reinterpret_cast<const bf16x8_t*>(pb + 8 * q);                                  \
    }                                                                                          \
    _Pragma("unroll") for (int q = 0; q < HBK / 16; ++q)                                       \
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[q], fb[q], acc, 0, 0, 0);             \
    if (do_colsum && tid < 64) { /* bias gradient: column sums of the staged (bf16) dy tile */ \
      const uint32_t* row = reinterpret_cast<const uint32_t*>(As + tid * HP);                  \
      _Pragma("unroll") for (int k = 0; k < HBK / 2; ++k) {                                    \
        const uint32_t w = row[k];                                                             \
        csum += __uint_as_float(w << 16) + __uint_as_float(w & 0xffff0000u);                   \
      }                                                                                        \
    }                                                                                          \
    __syncthreads();                                                                           \
  } while (0)
  for (int k0 = kbeg; k0 < kend; k0 += 2 * HBK) {
    H_STEP(ra0, rb0, k0 + 2 * HBK);
    if (k0 + HBK < kend) H_STEP(ra1, rb1, k0 + 3 * HBK);
  }
#undef H_STEP

#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    const int gm = m0 + wm * 32 + row;
    if (gm < p.M && gn < p.N) {
      float v = acc[r] + bias;
      if (p.relu) v = fmaxf(v, 0.f);
      v = mk[r] > 0.f ? v : 0.f;
      float* c = p.C + (size_t)gm * p.ldc + gn;
      if (p.atomic)
        atomic_add_f32(c, v);
      else
        *c = v;
    }
  }
  if (do_colsum && tid < 64 && m0 + tid < p.M) atomic_add_f32(p.colsum + m0 + tid, csum);
}

template <int HBK>
__global__ __launch_bounds__(256) void gemm_bf16op_multi_kernel(MultiArgs m) {
  __shared__ __attribute__((aligned(16))) uint16_t As[64 * (HBK + 8)];
  __shared__ __attribute__((aligned(16))) uint16_t Bs[64 * (HBK + 8)];
  int i = 0;
#pragma unroll
  for (int j = 1; j < MULTI_MAX; ++j)
    if (j < m.n && (int)blockIdx.x >= m.blk0[j]) i = j;
  const int local = (int)blockIdx.x - m.blk0[i];
  const int bx = local % m.gx[i], by = (local / m.gx[i]) % m.gy[i], bz = local / (m.gx[i] * m.gy[i]);
  switch (m.layout[i]) {
    case 0: gemm_bf16op_body<true, true, HBK>(m.g[i], bx, by, bz, As, Bs); break;
    case 1: gemm_bf16op_body<true, false, HBK>(m.g[i], bx, by, bz, As, Bs); break;
    default: gemm_bf16op_body<false, false, HBK>(m.g[i], bx, by, bz, As, Bs); break;
  }
}

// Tile configurations: 0 = 64x64 (4 waves), 1 = 32x64 (2 waves), 2 = 32x32 (1 wave), 3 = 64x32.
int g_cfg_override = -1;  // dvt_tune_set(0, cfg); > 0 also keeps the fit off the LDS-DMA ring

// The batch is small (2048 rows): pick the largest tile that still yields >= ~2 workgroups
// per CU worth of waves, so that barrier / load phases of one wave hide behind another's MFMAs.
int pick_cfg(int M, int N, int ksplits) {
  // Measured at the fit's shapes (M = 2048, N, K <= 768): the per-tile time is set by the
  // staging latency, not by the number of workgroups -- 64x64 wins everywhere (322.6 us/step vs
  // 340.2 / 333.1 for 32x64 / 32x32), so it is the default; smaller tiles only for tiny outputs.
  if (g_cfg_override >= 0 && g_cfg_override < 4) return g_cfg_override;
  (void)ksplits;
  if (M <= 32 || N <= 32) return 2;
  return 0;
}

// k-depth of the register-staged kernel: 64, 32 or 16 (dvt_tune_set(5, v)).  Default 32 (17 KB of LDS per workgroup):
// in the pipelined driver the fit shares every CU with a 136-KB ViT GEMM workgroup, and a fit
// kernel that does not fit beside it has to wait for CUs to drain (measured: 1.55 -> 1.72 images/s;
// the serial fit time is unchanged, 0.345 s).  64 re-enables the 96-KB LDS-DMA ring (dvt_gemm_f32_glds.hip).
int g_f32_bk = 32;

template <bool A_KC, bool B_KC, int WM, int WN, int BKT>
int launch_cfg(const GemmArgs& a, int ksplits, hipStream_t s) {
  dim3 grid(dvt_cdiv(a.N, 32 * WN), dvt_cdiv(a.M, 32 * WM), ksplits);
  DvtProbeScope probe(DVT_PROBE_FIT_GEMM, s, 2.0 * a.M * a.N * a.K);
  hipLaunchKernelGGL((gemm_f32_kernel<A_KC, B_KC, WM, WN, BKT>), grid, dim3(64 * WM * WN), 0, s, a);
  DVT_CHECK_LAUNCH();
  return 0;
}

template <bool A_KC, bool B_KC>
int launch(const GemmArgs& a, int ksplits, hipStream_t s) {
  constexpr int layout = A_KC ? (B_KC ? 0 : 1) : 2;
  if (g_f32_bk == 64 && g_cfg_override <= 0 && gemm_f32_glds_ok(a, layout)) return gemm_f32_glds_launch(a, layout, 3, ksplits, s);
  const int cfg = pick_cfg(a.M, a.N, ksplits);
  if (g_f32_bk == 16) return launch_cfg<A_KC, B_KC, 2, 2, 16>(a, ksplits, s);
  if (g_f32_bk == 32) return launch_cfg<A_KC, B_KC, 2, 2, 32>(a, ksplits, s);
  switch (cfg) {
    case 0: return launch_cfg<A_KC, B_KC, 2, 2, 64>(a, ksplits, s);
    case 1: return launch_cfg<A_KC, B_KC, 1, 2, 64>(a, ksplits, s);
    case 3: return launch_cfg<A_KC, B_KC, 2, 1, 64>(a, ksplits, s);
    default: return launch_cfg<A_KC, B_KC, 1, 1, 64>(a, ksplits, s);
  }
}

}  // namespace

// This unit's share of dvt_tune_set (dvt_tune.h)
int gemm_f32_tune(int key, int value) {
  if (key == 0) {
    g_cfg_override = value;
    return 0;
  }
  if (key == 5) {
    if (value != 16 && value != 32 && value != 64) return DVT_E_BADARG;
    g_f32_bk = value;
    return 0;
  }
  return DVT_TUNE_NOT_MINE;
}

int gemm_f32_staged_fwd(const DvtGemmF32Args& a, hipStream_t s) { return launch<true, true>(GemmArgs{a}, 1, s); }

int dvt_linear_group(const DvtLinearOp* ops, int n_ops, hipStream_t s, int bf16_operands) {
  if (!ops || n_ops < 1 || n_ops > MULTI_MAX) return DVT_E_BADARG;
  MultiArgs m{};
  m.n = n_ops;
  int blocks = 0;
  double flops = 0.0;
  for (int i = 0; i < n_ops; ++i) {
    const DvtLinearOp& o = ops[i];
    if (o.m <= 0 || o.n <= 0 || o.k <= 0 || (o.n & 3) || (o.k & 3)) return DVT_E_BADARG;
    int splits = 1;
    if (o.kind == 0) {
      m.g[i] = make_fwd(o.x, o.w, o.b, o.y, o.m, o.n, o.k, o.relu);
      m.layout[i] = 0;
    } else if (o.kind == 1) {
      m.g[i] = make_wgrad(o.dy, o.x, o.dw, o.db, o.m, o.n, o.k, &splits);
      m.layout[i] = 2;
    } else if (o.kind == 2) {
      m.g[i] = make_dgrad(o.dy, o.w, o.dx, o.relu_mask, o.m, o.n, o.k);
      m.layout[i] = 1;
    } else {
      return DVT_E_BADARG;
    }
    m.gx[i] = dvt_cdiv(m.g[i].N, 64);
    m.gy[i] = dvt_cdiv(m.g[i].M, 64);
    m.blk0[i] = blocks;
    blocks += m.gx[i] * m.gy[i] * splits;
    flops += 2.0 * o.m * o.n * o.k;
  }
  m.blk0[n_ops] = blocks;
  DvtProbeScope probe(DVT_PROBE_FIT_GEMM, s, flops);
  if (bf16_operands) {
    // BK = 32 (80 VGPRs, 10 KB of LDS): fits beside the extractor's workgroups; BK = 64 (146 VGPRs)
    // is equally fast alone (214 vs 215 us/step) and slower in the pipeline (2.09 vs 2.12 images/s)
    if (g_f32_bk == 64)
      hipLaunchKernelGGL(gemm_bf16op_multi_kernel<64>, dim3(blocks), dim3(256), 0, s, m);
    else
      hipLaunchKernelGGL(gemm_bf16op_multi_kernel<32>, dim3(blocks), dim3(256), 0, s, m);
  } else if (g_f32_bk == 16)
    hipLaunchKernelGGL(gemm_f32_multi_kernel<16>, dim3(blocks), dim3(256), 0, s, m);
  else if (g_f32_bk == 32)
    hipLaunchKernelGGL(gemm_f32_multi_kernel<32>, dim3(blocks), dim3(256), 0, s, m);
  else
    hipLaunchKernelGGL(gemm_f32_multi_kernel<64>, dim3(blocks), dim3(256), 0, s, m);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int dvt_linear_fwd(const float* x, const float* w, const float* b, float* y, int m,
                              int n, int k, int relu, void* stream) {
  if (!x || !w || !y || m < 0 || n <= 0 || k <= 0 || (k & 3) || (n & 3)) return DVT_E_BADARG;
  if (m == 0) return 0;
  return launch<true, true>(make_fwd(x, w, b, y, m, n, k, relu), 1, (hipStream_t)stream);
}

extern "C" int dvt_linear_bwd(const float* dy, const float* x, const float* w, float* dw,
                              float* db, float* dx, const float* relu_mask, int m, int n, int k,
                              void* stream) {
  if (!dy || m < 0 || n <= 0 || k <= 0 || (k & 3) || (n & 3)) return DVT_E_BADARG;
  if (m == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (dw != nullptr) {
    if (!x) return DVT_E_BADARG;
    int splits = 1;
    const GemmArgs a = make_wgrad(dy, x, dw, db, m, n, k, &splits);
    int rc = launch<false, false>(a, splits, s);
    if (rc) return rc;
  } else if (db != nullptr) {
    return DVT_E_BADARG;  // db is produced by the wgrad launch
  }
  if (dx != nullptr) {
    if (!w) return DVT_E_BADARG;
    int rc = launch<true, false>(make_dgrad(dy, w, dx, relu_mask, m, n, k), 1, s);
    if (rc) return rc;
  }
  return 0;
}
