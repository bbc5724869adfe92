// Exact-fp32 GEMM on the LDS-DMA ring (64 x 64 x 64 tile, 2 or 3 stages): dvt_gemm_f32_ex, the building block of the stage-2
// and stage-3 trainers, the fp32 extractor's fallback (dvt_linear_fwd_big, dvt_gemm_f32_big.hip) and the stage-1 fit when
// dvt_tune_set(5, 64) selects it (dvt_gemm_f32.hip) -- the last two through gemm_f32_glds_launch.  The batched small-k kernel
// lives here too: dvt_gemm_f32_ex is its only caller; its body is the register-staged one of dvt_gemm_f32_dev.h.
#include "dvt_gemm_f32_dev.h"
#include "dvt_tune.h"

namespace {

// ==========================================================================================
// 3-stage LDS-DMA variant (used when K % 64 == 0 and row-contiguous operands are 64-aligned).
// PMC evidence for the register-staged kernel (dvt_gemm_f32.hip) at the fit's shapes: L2 hit rate 43 % (the
// operands were just written by other XCDs' kernels), waves 45-54 % in s_waitcnt, MFMA pipe
// ~13 % busy -> latency-bound with one tile in flight.  Here global_load_lds keeps TWO 32-KB
// stages in flight per workgroup behind the one being multiplied: one raw s_barrier per
// k-tile and a counted `s_waitcnt vmcnt(8)` (8 DMA instructions per thread per stage).
// LDS image is lane-linear; for k-contiguous operands the 16-B chunk index of a 256-B row is
// XOR-ed with (row & 15) through the SOURCE address, and the b128 fragment reads apply the
// same XOR (conflict-free: the 16 rows of a lane group hit 16 distinct slots).
// ==========================================================================================
constexpr int G3_STAGE_FLOATS = 2 * 64 * BK;  // A tile + B tile, 64 rows/cols x 64 k = 32 KB

template <bool KCONTIG>
__device__ __forceinline__ void stage_f32(const float* __restrict__ X, int ld, int r0, int Rmax,
                                          int k0, float* lds, int wave, int lane) {
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int s = it * 256 + wave * 64 + lane;  // 16-B slot in the 16-KB tile
    const float* src;
    if (KCONTIG) {
      const int row = s >> 4, cp = s & 15, c = cp ^ (row & 15);
      src = X + (size_t)min(r0 + row, Rmax - 1) * ld + k0 + c * 4;  // rows >= Rmax: clamped, masked at the store
    } else {
      const int k = s >> 4, cq = s & 15;
      src = X + (size_t)(k0 + k) * ld + r0 + cq * 4;
    }
    glds16f(src, lds + (it * 256 + wave * 64) * 4);
  }
}

template <bool KCONTIG>
__device__ __forceinline__ void frags_f32(const float* __restrict__ S, int row, int kh,
                                          float (&f)[BK / 2]) {
  if (KCONTIG) {
#pragma unroll
    for (int q = 0; q < BK / 8; ++q) {
      const int chunk = (kh * (BK / 8) + q) ^ (row & 15);
      const float4 v = *reinterpret_cast<const float4*>(S + row * BK + chunk * 4);
      f[4 * q + 0] = v.x;
      f[4 * q + 1] = v.y;
      f[4 * q + 2] = v.z;
      f[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) f[kk] = S[(kh * (BK / 2) + kk) * 64 + row];
  }
}

// NS = 3 stages (96 KB, one workgroup per CU, loads two k-tiles ahead) or 2 stages (64 KB, TWO workgroups per CU,
// loads one k-tile ahead): with one workgroup per CU every k-tile exposes its barrier + fragment-read latency
// (the MFMA pipe idles ~45 % of the time); a second resident workgroup fills those gaps.
template <bool A_KC, bool B_KC, int NS = 3>
__device__ __forceinline__ void gemm_f32_glds_body(const GemmArgs& p, int bz, float* __restrict__ smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
  const int kbeg = bz * p.kchunk;
  const int kend = min(p.K, kbeg + p.kchunk);
  if (kbeg >= kend) return;
  const int nk = (kend - kbeg) / BK;

  floatx16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float csum = 0.f;
  const bool do_colsum = (!A_KC) && p.colsum != nullptr && blockIdx.x == 0;

#define G3_ISSUE(kt)                                                                          \
  do {                                                                                        \
    float* st_ = smem + ((kt) % NS) * G3_STAGE_FLOATS;                                        \
    stage_f32<A_KC>(p.A, p.lda, m0, p.M, kbeg + (kt) * BK, st_, wave, lane);                  \
    stage_f32<B_KC>(p.B, p.ldb, n0, p.N, kbeg + (kt) * BK, st_ + 64 * BK, wave, lane);        \
  } while (0)
  G3_ISSUE(0);
  if (NS == 3 && nk > 1) G3_ISSUE(1);
  for (int kt = 0; kt < nk; ++kt) {
    if (NS == 3 && kt + 1 < nk)
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (kt + NS - 1 < nk) G3_ISSUE(kt + NS - 1);
    const float* As = smem + (kt % NS) * G3_STAGE_FLOATS;
    const float* Bs = As + 64 * BK;
    const int ar = wm * 32 + (lane & 31), bc = wn * 32 + (lane & 31), kh = lane >> 5;
    float fa[BK / 2], fb[BK / 2];
    frags_f32<A_KC>(As, ar, kh, fa);
    frags_f32<B_KC>(Bs, bc, kh, fb);
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk], fb[kk], acc, 0, 0, 0);
    if (do_colsum && tid < 64) {
#pragma unroll 8
      for (int k = 0; k < BK; ++k) csum += As[k * 64 + tid];
    }
  }
#undef G3_ISSUE

  const int gn = n0 + wn * 32 + (lane & 31);
  const float bias = (p.bias != nullptr && gn < p.N) ? p.bias[gn] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    const int gm = m0 + wm * 32 + row;
    if (gm < p.M && gn < p.N) {
      float v = acc[r] + bias;
      if (p.relu) v = fmaxf(v, 0.f);
      if (p.mask != nullptr) v = p.mask[(size_t)gm * p.ldmask + gn] > 0.f ? v : 0.f;
      float* c = p.C + (size_t)gm * p.ldc + gn;
      if (p.atomic)
        atomic_add_f32(c, v);
      else
        *c = v;
    }
  }
  if (do_colsum && tid < 64 && m0 + tid < p.M) atomic_add_f32(p.colsum + m0 + tid, csum);
}

template <bool A_KC, bool B_KC, int NS = 3>
__global__ __launch_bounds__(256) void gemm_f32_glds_kernel(GemmArgs p) {
  __shared__ __attribute__((aligned(16))) float smem[NS * G3_STAGE_FLOATS];  // 96 / 64 KB, one LDS object
  gemm_f32_glds_body<A_KC, B_KC, NS>(p, blockIdx.z, smem);
}

template <bool A_KC, bool B_KC, int NS = 3>
__global__ __launch_bounds__(256) void gemm_f32_glds_batched_kernel(GemmArgs p, BatchDims d) {
  __shared__ __attribute__((aligned(16))) float smem[NS * G3_STAGE_FLOATS];
  const int b0 = blockIdx.z / d.nb1, b1 = blockIdx.z - b0 * d.nb1;
  GemmArgs q = p;
  q.A = p.A + b0 * d.sA0 + b1 * d.sA1;
  q.B = p.B + b0 * d.sB0 + b1 * d.sB1;
  q.C = p.C + b0 * d.sC0 + b1 * d.sC1;
  gemm_f32_glds_body<A_KC, B_KC, NS>(q, 0, smem);
}

// Single-k-tile problems (q k^T and dO v^T of the stage-2 attention: K = 64) gain nothing from the 3-stage ring, and
// its 96 KB of LDS hold a CU to ONE workgroup whose only tile is pure load -> MFMA -> store latency (measured:
// 27 TF/s).  The register-staged body needs 35 KB: four workgroups per CU overlap each other's latencies.
template <bool A_KC, bool B_KC>
__global__ __launch_bounds__(256) void gemm_f32_batched_small_k_kernel(GemmArgs p, BatchDims d) {
  __shared__ __attribute__((aligned(16))) float As[Tile<A_KC, 64, 256, 64>::LDS_FLOATS];
  __shared__ __attribute__((aligned(16))) float Bs[Tile<B_KC, 64, 256, 64>::LDS_FLOATS];
  const int b0 = blockIdx.z / d.nb1, b1 = blockIdx.z - b0 * d.nb1;
  GemmArgs q = p;
  q.A = p.A + b0 * d.sA0 + b1 * d.sA1;
  q.B = p.B + b0 * d.sB0 + b1 * d.sB1;
  q.C = p.C + b0 * d.sC0 + b1 * d.sC1;
  if (p.smul != nullptr) {
    q.smul = p.smul + b0 * d.sC0 + b1 * d.sC1;
    q.rowsub = p.rowsub + (size_t)blockIdx.z * p.M;
  }
  gemm_f32_body<A_KC, B_KC, 2, 2, 64>(q, blockIdx.x, blockIdx.y, 0, As, Bs);
}

int g_f32_glds = 1;       // dvt_tune_set(4, 0): the fit never takes the ring (always its register-staged kernel)
int g_f32_ex_stages = 2;  // dvt_tune_set(4, 2 / 3): LDS stages of the stage-2 GEMMs (dvt_gemm_f32_ex) and of dvt_linear_fwd_big's fallback

// one problem (d == nullptr) or a batch of them: the kernel of this layout and ring depth
template <int NS>
void launch_ring(const GemmArgs& a, int layout, const BatchDims* d, dim3 grid, hipStream_t s) {
  if (d) {
    if (layout == 0)
      hipLaunchKernelGGL((gemm_f32_glds_batched_kernel<true, true, NS>), grid, dim3(256), 0, s, a, *d);
    else if (layout == 1)
      hipLaunchKernelGGL((gemm_f32_glds_batched_kernel<true, false, NS>), grid, dim3(256), 0, s, a, *d);
    else
      hipLaunchKernelGGL((gemm_f32_glds_batched_kernel<false, false, NS>), grid, dim3(256), 0, s, a, *d);
  } else {
    if (layout == 0)
      hipLaunchKernelGGL((gemm_f32_glds_kernel<true, true, NS>), grid, dim3(256), 0, s, a);
    else if (layout == 1)
      hipLaunchKernelGGL((gemm_f32_glds_kernel<true, false, NS>), grid, dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL((gemm_f32_glds_kernel<false, false, NS>), grid, dim3(256), 0, s, a);
  }
}

}  // namespace

// This unit's share of dvt_tune_set: key 4, after the 128 x 128 unit has taken its two values (dvt_tune.h)
int gemm_f32_glds_tune(int key, int value) {
  if (key != 4) return DVT_TUNE_NOT_MINE;
  if (value == 2 || value == 3)
    g_f32_ex_stages = value;
  else
    g_f32_glds = value;
  return 0;
}

bool gemm_f32_glds_ok(const DvtGemmF32Args& a, int layout) {
  if (!g_f32_glds || (a.K % BK) || (a.kchunk % BK)) return false;
  if (layout == 2 && (a.M % 64)) return false;  // row-contiguous A
  if (layout != 0 && (a.N % 64)) return false;  // row-contiguous B
  return a.M >= 1 && a.N >= 1;
}

int gemm_f32_glds_launch(const DvtGemmF32Args& a, int layout, int stages, int ksplits, hipStream_t s) {
  const dim3 grid(dvt_cdiv(a.N, 64), dvt_cdiv(a.M, 64), ksplits);
  DvtProbeScope probe(DVT_PROBE_FIT_GEMM, s, 2.0 * a.M * a.N * a.K);
  if ((stages ? stages : g_f32_ex_stages) == 2)
    launch_ring<2>(GemmArgs{a}, layout, nullptr, grid, s);
  else
    launch_ring<3>(GemmArgs{a}, layout, nullptr, grid, s);
  DVT_CHECK_LAUNCH();
  return 0;
}

// General exact-fp32 GEMM for the stage-2 trainer (dvt_stage2.hip): any of the three operand layouts with
// explicit leading dimensions, optional (image, head) batching, optional atomic accumulation with a k-split.
// Always the LDS-DMA ring (there is no extractor to share the CUs with in stage 2), so the shapes
// must be whole 64-tiles where that kernel needs them (checked).
int dvt_gemm_f32_ex(const DvtGemmEx* g, hipStream_t s) {
  if (!g || !g->A || !g->B || !g->C || g->M <= 0 || g->N <= 0 || g->K <= 0) return DVT_E_BADARG;
  GemmArgs a{};
  a.A = g->A; a.B = g->B; a.C = g->C;
  a.M = g->M; a.N = g->N; a.K = g->K;
  a.lda = g->lda; a.ldb = g->ldb; a.ldc = g->ldc;
  a.bias = g->bias;
  a.colsum = g->layout == 2 ? g->colsum : nullptr;
  a.atomic = g->accumulate;
  if (g->smul != nullptr) {  // softmax-backward epilogue: the batched small-k kernel only
    const int nb_ = (g->nb0 > 0 ? g->nb0 : 1) * (g->nb1 > 0 ? g->nb1 : 1);
    if (!g->rowsub || g->layout != 0 || nb_ <= 1 || g->K > BK || g->accumulate) return DVT_E_BADARG;
    a.smul = g->smul;
    a.rowsub = g->rowsub;
    a.oscale = g->oscale;
  }
  if (a.K % BK) return DVT_E_BADARG;
  const bool a_kc = g->layout != 2, b_kc = g->layout == 0;
  if ((!a_kc && (a.M % 64)) || (!b_kc && (a.N % 64)) || (a.lda & 3) || (a.ldb & 3)) return DVT_E_BADARG;
  const int nb = (g->nb0 > 0 ? g->nb0 : 1) * (g->nb1 > 0 ? g->nb1 : 1);
  int splits = 1;
  a.kchunk = a.K;
  if (g->accumulate && nb == 1) {  // split the reduction so that ~1024 workgroups exist (one atomic per split)
    const int tiles = dvt_cdiv(a.M, 64) * dvt_cdiv(a.N, 64), ktiles = a.K / BK;
    splits = dvt_cdiv(1024, tiles);
    if (splits > ktiles / 4) splits = ktiles / 4;
    if (splits < 1) splits = 1;
    a.kchunk = dvt_cdiv(ktiles, splits) * BK;
    splits = dvt_cdiv(a.K, a.kchunk);
  }
  if (nb > 65535 || splits > 65535) return DVT_E_BADARG;
  if (nb <= 1) return gemm_f32_glds_launch(a, g->layout, 0, splits, s);
  const dim3 grid(dvt_cdiv(a.N, 64), dvt_cdiv(a.M, 64), nb);
  const BatchDims d{g->nb1 > 0 ? g->nb1 : 1, g->sA0, g->sA1, g->sB0, g->sB1, g->sC0, g->sC1};
  DvtProbeScope probe(DVT_PROBE_FIT_GEMM, s, 2.0 * a.M * a.N * a.K * nb);
  if (a.K <= BK && g->layout == 0)
    hipLaunchKernelGGL((gemm_f32_batched_small_k_kernel<true, true>), grid, dim3(256), 0, s, a, d);
  else if (g_f32_ex_stages == 2)
    launch_ring<2>(a, g->layout, &d, grid, s);
  else
    launch_ring<3>(a, g->layout, &d, grid, s);
  DVT_CHECK_LAUNCH();
  return 0;
}

// ---- component entry point for tests (include/dvt_parts.h): a forwarder only, no kernel and no launch of its own ----
#include "../../include/dvt_parts.h"
static_assert(sizeof(DvtPartsGemmEx) == 160, "DvtPartsGemmEx: explicit padding, mirrored by dvt_amd/_lib.py PartsGemmEx");

extern "C" int dvt_parts_gemm_ex(const DvtPartsGemmEx* p, void* stream) {
  if (!p || p->layout < 0 || p->layout > 2 || p->ldc < p->N || p->nb0 < 0 || p->nb1 < 0) return DVT_E_BADARG;
  DvtGemmEx g{};
  g.layout = p->layout;
  g.A = p->A; g.B = p->B; g.C = p->C;
  g.M = p->M; g.N = p->N; g.K = p->K;
  g.lda = p->lda; g.ldb = p->ldb; g.ldc = p->ldc;
  g.bias = p->bias;
  g.colsum = p->colsum;
  g.accumulate = p->accumulate;
  g.nb0 = p->nb0; g.nb1 = p->nb1;
  g.sA0 = p->sA0; g.sA1 = p->sA1; g.sB0 = p->sB0; g.sB1 = p->sB1; g.sC0 = p->sC0; g.sC1 = p->sC1;
  g.smul = p->smul;
  g.rowsub = p->rowsub;
  g.oscale = p->oscale;
  return dvt_gemm_f32_ex(&g, (hipStream_t)stream);  // (every check of its own runs before its launch)
}
