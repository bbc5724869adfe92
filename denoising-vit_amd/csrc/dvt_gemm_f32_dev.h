// What the units of the exact-fp32 GEMM share (v_mfma_f32_32x32x2_f32: 64 FLOP/clk/SIMD, bitwise an fmaf chain):
//   dvt_gemm_f32.hip       register-staged 64 x 64 (32 x 64, 32 x 32, 64 x 32) tile, BK 16 / 32 / 64: the stage-1 fit
//   dvt_gemm_f32_glds.hip  LDS-DMA 64 x 64 x 64 ring of 2 or 3 stages (+ the batched small-k kernel): stages 2 / 3, dvt_gemm_f32_ex
//   dvt_gemm_f32_big.hip   128 x 128 x 32 tile: the fp32 extractor and stages 2 / 3
// One argument block and one operand convention serve all of them; the operands of a linear layer's three contractions differ
// only in which index is contiguous in memory:
//   forward  y = x . w^T      A = x  [m][k] k-contiguous   B = w  [n][k] k-contiguous     (layout 0)
//   dgrad    dx = dy . w      A = dy [m][n] k-contiguous   B = w  [n][k] row-contiguous   (layout 1)
//   wgrad    dw = dy^T . x    A = dy [b][n] row-contiguous B = x  [b][k] row-contiguous   (layout 2)
// Every __global__ template is instantiated in ONE unit; a host function that needs another unit's kernel calls that unit's
// launcher (declared at the end).
#pragma once
#include "dvt_common.h"

typedef float floatx16 __attribute__((ext_vector_type(16)));

// The members of GemmArgs as a type with external linkage: what a launcher takes across units.  The kernels' parameter stays
// (anonymous namespace)::GemmArgs, which derives from it without adding a member (same bytes, same kernel-argument loads,
// same mangled kernel names in every unit).
struct DvtGemmF32Args {
  const float* A;
  const float* B;
  float* C;
  int M, N, K;
  int lda, ldb, ldc;
  const float* bias;  // [N] added per output column
  const float* mask;  // [M, ldmask]: output multiplied by (mask > 0)
  int ldmask;
  float* colsum;  // [M]: += sum_k A(m,k), written by the n-tile-0 blocks (A row-contiguous only)
  int relu;
  int kchunk;  // K range per blockIdx.z (multiple of BK)
  int atomic;  // accumulate into C with atomics
  // gemm_f32_big_kernel only (the fp32 extractor's fused epilogues): 1 = exact-erf GELU of (acc + bias); 2 = residual,
  // C[m][n] += gamma[n] * (acc + bias[n]) (timm Block: x = x + ls(f(norm(x))))
  int epi;
  const float* gamma;
  // gemm_f32_body, set by the batched small-k kernel only: C = oscale * smul[m][n] * (acc - rowsub[m]) -- the softmax backward
  // dS = scale P (.) (dP - rowsum(dP (.) P)) as the epilogue of dP = dO V^T, with rowsum(dP (.) P) = dO . O handed in
  const float* smul;
  const float* rowsub;
  float oscale;
};

namespace {

// BK = 64: 32 MFMAs (2048 cycles) per staged tile -- with BK = 32 every k-tile cost ~1 us, twice
// its MFMA time, because the single prefetched tile's L2 latency was only half hidden.
constexpr int BK = 64;
constexpr int LDK = BK + 4;  // [row][k] layout: rows stay 16-B aligned for b128 accesses; a 16-lane
                            // group reading 16 B at a 272-B row stride covers all 16 bank slots

struct GemmArgs : DvtGemmF32Args {};

// Batched form (stage-2 attention: one problem per (image, head)): blockIdx.z = b0 * nb1 + b1 selects
// the operand bases, no k-split.
struct BatchDims {
  int nb1;
  long long sA0, sA1, sB0, sB1, sC0, sC1;
};

// One LDS-DMA instruction: 16 B per lane, lane-linear behind the wave's LDS base (the ring and the 128 x 128 kernels)
__device__ __forceinline__ void glds16f(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// Operand tile of R rows x BK: R*BK/4 float4, spread over NT threads.  Staged through LDS so that global reads are 16-B
// coalesced and the MFMA fragment reads (lane l: A[l&31][l>>5], B[l>>5][l&31]) are conflict-free:
//   k-contiguous operand  -> LDS [row][k] with leading dimension BK+4
//   row-contiguous operand-> LDS [k][row] with leading dimension R
// BK is a template parameter of the register-staged kernel: 64 by default, 16 (10 KB of LDS per workgroup) when
// the fit shares the GPU with the ViT extractor, whose 136-144 KB workgroups leave only 16-24 KB
// of a CU's LDS free (co-residency instead of waiting for CUs to drain).
template <bool KCONTIG, int R, int NT, int BK>
struct Tile {
  static constexpr int LDK = BK + 4;
  static constexpr int NF4 = R * BK / 4;
  static constexpr int ITERS = (NF4 + NT - 1) / NT;
  static constexpr int LDS_FLOATS = KCONTIG ? R * LDK : BK * R;

  __device__ static __forceinline__ void load(const float* __restrict__ X, int ld, int r0, int Rmax,
                                              int k0, int kend, int tid, float4 regs[ITERS]) {
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const int f = tid + NT * i;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (NF4 % NT == 0 || f < NF4) {
        if (KCONTIG) {
          const int r = f / (BK / 4), kq = f % (BK / 4);
          const int gr = r0 + r, gk = k0 + 4 * kq;
          if (gr < Rmax && gk < kend) v = *reinterpret_cast<const float4*>(X + (size_t)gr * ld + gk);
        } else {
          const int k = f / (R / 4), rq = f % (R / 4);
          const int gk = k0 + k, gr = r0 + 4 * rq;
          if (gk < kend && gr < Rmax) v = *reinterpret_cast<const float4*>(X + (size_t)gk * ld + gr);
        }
      }
      regs[i] = v;
    }
  }

  __device__ static __forceinline__ void store(float* __restrict__ S, int tid,
                                               const float4 regs[ITERS]) {
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const int f = tid + NT * i;
      if (NF4 % NT == 0 || f < NF4) {
        if (KCONTIG) {
          const int r = f / (BK / 4), kq = f % (BK / 4);
          *reinterpret_cast<float4*>(S + r * LDK + 4 * kq) = regs[i];
        } else {
          const int k = f / (R / 4), rq = f % (R / 4);
          *reinterpret_cast<float4*>(S + k * R + 4 * rq) = regs[i];
        }
      }
    }
  }

  // All BK/2 = 32 fragment values of one lane for this tile.  MFMA step kk uses k index
  // kh*32 + kk (kh = lane >> 5): any bijection of k is valid as long as A and B agree, and this
  // one makes a lane's values CONTIGUOUS in the k-contiguous layout (8 x ds_read_b128).
  __device__ static __forceinline__ void frags(const float* __restrict__ S, int row, int kh,
                                               float (&f)[BK / 2]) {
    if (KCONTIG) {
      const float4* p = reinterpret_cast<const float4*>(S + row * LDK + kh * (BK / 2));
#pragma unroll
      for (int q = 0; q < BK / 8; ++q) {
        const float4 v = p[q];
        f[4 * q + 0] = v.x;
        f[4 * q + 1] = v.y;
        f[4 * q + 2] = v.z;
        f[4 * q + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int kk = 0; kk < BK / 2; ++kk) f[kk] = S[(kh * (BK / 2) + kk) * R + row];
    }
  }
};

// WM x WN waves, each owning one 32x32 accumulator: tile (32*WM) x (32*WN).
// Body shared by the fit's single-problem and grouped kernels (dvt_gemm_f32.hip) and by the batched small-k kernel
// (dvt_gemm_f32_glds.hip); explicit block coordinates.
template <bool A_KC, bool B_KC, int WM, int WN, int BK>
__device__ __forceinline__ void gemm_f32_body(const GemmArgs& p, int bx, int by, int bz,
                                              float* __restrict__ As, float* __restrict__ Bs) {
  constexpr int NT = 64 * WM * WN, BM = 32 * WM, BN = 32 * WN;
  using TA = Tile<A_KC, BM, NT, BK>;
  using TB = Tile<B_KC, BN, NT, BK>;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int n0 = bx * BN, m0 = by * BM;
  const int kbeg = bz * p.kchunk;
  const int kend = min(p.K, kbeg + p.kchunk);
  if (kbeg >= kend) return;

  floatx16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float csum = 0.f;
  const bool do_colsum = (!A_KC) && p.colsum != nullptr && bx == 0;

  float4 ra[TA::ITERS], rb[TB::ITERS];
  TA::load(p.A, p.lda, m0, p.M, kbeg, kend, tid, ra);
  TB::load(p.B, p.ldb, n0, p.N, kbeg, kend, tid, rb);
  for (int k0 = kbeg; k0 < kend; k0 += BK) {
    TA::store(As, tid, ra);
    TB::store(Bs, tid, rb);
    __syncthreads();
    if (k0 + BK < kend) {  // prefetch the next tile while the MFMAs run
      TA::load(p.A, p.lda, m0, p.M, k0 + BK, kend, tid, ra);
      TB::load(p.B, p.ldb, n0, p.N, k0 + BK, kend, tid, rb);
    }
    // Fragments of the whole tile first, then 32 MFMAs back to back: the compiler otherwise
    // re-used one register pair and waited lgkmcnt(0) on a fresh ds_read every 2 dependent
    // MFMAs (each k-tile cost ~2x its MFMA time).
    const int ar = wm * 32 + (lane & 31), bc = wn * 32 + (lane & 31), kh = lane >> 5;
    float fa[BK / 2], fb[BK / 2];
    TA::frags(As, ar, kh, fa);
    TB::frags(Bs, bc, kh, fb);
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk], fb[kk], acc, 0, 0, 0);
    if (do_colsum && tid < BM) {
#pragma unroll 8
      for (int k = 0; k < BK; ++k) csum += As[k * BM + tid];
    }
    __syncthreads();
  }

  // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
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
      if (p.smul != nullptr) v = p.oscale * p.smul[(size_t)gm * p.ldc + gn] * (v - p.rowsub[gm]);
      float* c = p.C + (size_t)gm * p.ldc + gn;
      if (p.atomic)
        atomic_add_f32(c, v);
      else
        *c = v;
    }
  }
  if (do_colsum && tid < BM && m0 + tid < p.M) atomic_add_f32(p.colsum + m0 + tid, csum);
}

// ---- GemmArgs builders for the three contractions of a linear layer ----
inline GemmArgs make_fwd(const float* x, const float* w, const float* b, float* y, int m, int n, int k,
                         int relu) {
  GemmArgs a{};
  a.A = x; a.B = w; a.C = y;
  a.M = m; a.N = n; a.K = k;
  a.lda = k; a.ldb = k; a.ldc = n;
  a.bias = b; a.relu = relu;
  a.kchunk = (k + 63) / 64 * 64;
  return a;
}

// dw[n,k] += sum_b dy[b,n] * x[b,k]; the batch reduction is split so that ~384 workgroups exist
inline GemmArgs make_wgrad(const float* dy, const float* x, float* dw, float* db, int m, int n, int k,
                           int* splits_out) {
  GemmArgs a{};
  a.A = dy; a.B = x; a.C = dw;
  a.M = n; a.N = k; a.K = m;
  a.lda = n; a.ldb = k; a.ldc = k;
  a.colsum = db;
  a.atomic = 1;
  const int tiles = dvt_cdiv(n, 64) * dvt_cdiv(k, 64);
  const int ktiles = dvt_cdiv(m, 64);
  int splits = dvt_cdiv(384, tiles);  // every split costs one fp32 atomic per output element
  if (splits > ktiles / 2) splits = ktiles / 2;
  if (splits < 1) splits = 1;
  a.kchunk = dvt_cdiv(ktiles, splits) * 64;
  *splits_out = dvt_cdiv(m, a.kchunk);
  return a;
}

inline GemmArgs make_dgrad(const float* dy, const float* w, float* dx, const float* relu_mask, int m,
                           int n, int k) {
  GemmArgs a{};
  a.A = dy; a.B = w; a.C = dx;
  a.M = m; a.N = k; a.K = n;
  a.lda = n; a.ldb = k; a.ldc = k;
  a.mask = relu_mask; a.ldmask = k;
  a.kchunk = (n + 63) / 64 * 64;
  return a;
}

}  // namespace

// ---- host launchers that cross units (not part of the C ABI) ----
// dvt_gemm_f32_glds.hip: the ring on one problem of the given operand layout, grid (N / 64, M / 64, ksplits).
// gemm_f32_glds_ok: whole k-tiles, row-contiguous operands whose 64-wide tile never runs past the row end, and the ring not
// switched off (dvt_tune_set(4, 0)).  stages: 2 or 3, 0 = the depth of dvt_tune_set(4, 2 / 3).
bool gemm_f32_glds_ok(const DvtGemmF32Args& a, int layout);
int gemm_f32_glds_launch(const DvtGemmF32Args& a, int layout, int stages, int ksplits, hipStream_t s);
// dvt_gemm_f32.hip: a forward layer (layout 0) as dvt_linear_fwd runs it, by the fit's knobs
int gemm_f32_staged_fwd(const DvtGemmF32Args& a, hipStream_t s);
