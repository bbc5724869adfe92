// The bf16 GEMM family of the ViT extractor for gfx950: C[M,N] = A[M,K] . W[N,K]^T, bf16 operands on
// v_mfma_f32_16x16x32_bf16, fp32 accumulation, one fused epilogue per use (dvt_vit_epilogue.h; EPI_* in dvt_vit_dev.h).
//
// Kernels the product launches from here, chosen by launch_gemm<EPI> from the shape and the schedule (dvt_tune_set(1, 4 / 3 / 1)):
//   gemm_bf16_kernel_8p<EPI, false, 0, KPOL>  256 x 256 tile, 8 waves, 8-phase half-tile ring (the default wherever M and N are
//                                             whole 256-tiles and the k-tiles pair up: every GEMM of a ViT-B / L / g block and
//                                             the patch embedding); KPOL = the epilogue cache policy as an instruction form
//   gemm_bf16_kernel_pp<EPI>                  256 x 128 tile, 8 waves, three-stage ping-pong: N % 256 != 0 (ViT-S, dim 384)
//   gemm_bf16_kernel<EPI>                     128 x 128 tile, 4 waves, two LDS stages: everything else (M % 256 != 0)
// Operands are staged with global_load_lds (16 B per lane, XOR-swizzled through the SOURCE address); tile order and XCD column
// sets: dvt_tile_map.h.  Host side: the GEMM knobs (g_vit_*; vit_gemm_tune), launch_gemm<EPI> with its per-shape defaults,
// and the dvt_vit_gemm_* entry points of include/dvt_vit.h.
// The developer build (-DDVT_LAB) adds the superseded / experimental kernels of lab/ and their dispatch (lab_launch_gemm,
// lab_gemm_tune: lab/dvt_vit_lab.inc); the product library contains none of it.
#include "dvt_vit_dev.h"
#include "dvt_vit_epilogue.h"

namespace {

// ======================================================================================
// GEMM  C[M,N] = A[M,K] . W[N,K]^T   (both operands K-contiguous bf16)
// ======================================================================================
// GEMM schedule (dvt_tune_set(1, v)).  4 (default): 256x256 8-phase half-tile ring where M and N are whole
// 256-tiles, else 3; 3: 256x128 ping-pong where M is a whole 256-tile, else 1; 1: 128x128 two-stage.
// Every selectable schedule computes the same result (tests/test_gpu_vit.py runs them all).
// Builds with -DDVT_LAB (tools/build_lab.py -> libdvt_hip_lab.so, never loaded by dvt_amd) add the superseded /
// experimental schedules of lab/: 0 256x256 two-stage, 2 256x128 lock-step, 5 "8m", 10 "8h", 6..9 the 4-wave
// persistent kernel, plus the timing builds; the product library rejects those values (DVT_E_BADARG).
int g_vit_gemm_variant = 4;
constexpr int STAGE_BYTES = (GBM + GBN) * GBK * 2;  // 32 KB

// async global -> LDS copy of 16 B per lane; the LDS address is wave-uniform base + lane*16
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)gsrc,
      (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// Stage one 128x64 bf16 tile (rows r0.., k0..) into `lds` (16 KB, rows of 128 B).  The LDS
// image is lane-linear; the 16-B chunk index inside a row is XOR-ed with (row & 7) by
// permuting the SOURCE address, and the fragment reads apply the same XOR.
__device__ __forceinline__ void stage_tile(const bf16_t* __restrict__ X, int ld, int r0, int k0,
                                           char* lds, int wave, int lane) {
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int s = it * 256 + wave * 64 + lane;  // LDS slot (16 B units)
    const int row = s >> 3, cp = s & 7;
    const int c = cp ^ (row & 7);
    glds16(X + (size_t)(r0 + row) * ld + k0 + c * 8, lds + (it * 256 + wave * 64) * 16);
  }
}

__device__ __forceinline__ bf16x8 read_frag(const char* lds, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(lds + row * 128 + ((chunk ^ (row & 7)) << 4));
}

template <int EPI>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(GemmBArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const TileMap tm = map_tile(blockIdx.x, gridDim.x, p.M / GBM, p.N / GBN, p.group);
  const int m0 = tm.m * GBM, n0 = tm.n * GBN;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nk = p.K / GBK;
  stage_tile(p.A, p.K, m0, 0, smem, wave, lane);
  stage_tile(p.W, p.K, n0, 0, smem + GBM * GBK * 2, wave, lane);
  __syncthreads();  // waits vmcnt(0) for the LDS-DMA before releasing the workgroup
  for (int kt = 0; kt < nk; ++kt) {
    char* cur = smem + (kt & 1) * STAGE_BYTES;
    char* nxt = smem + ((kt + 1) & 1) * STAGE_BYTES;
    if (kt + 1 < nk) {
      stage_tile(p.A, p.K, m0, (kt + 1) * GBK, nxt, wave, lane);
      stage_tile(p.W, p.K, n0, (kt + 1) * GBK, nxt + GBM * GBK * 2, wave, lane);
    }
    const char* As = cur;
    const char* Bs = cur + GBM * GBK * 2;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 a[4], b[4];
      const int chunk = ks * 4 + (lane >> 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = read_frag(As, wm * 64 + i * 16 + (lane & 15), chunk);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = read_frag(Bs, wn * 64 + j * 16 + (lane & 15), chunk);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();  // next stage landed (vmcnt(0)) and everyone is done reading `cur`
  }

  gemm_epilogue<EPI>(p, acc, m0, n0, wm, wn, lane);
}

// ---- 256x128x64 tile, 8 waves (4 x 2, 64x64 each), 3 LDS stages, counted vmcnt: the kernel of shapes
// with N % 256 != 0 (ViT-S: dim 384) -------------------------------------------------------------
// The loads of stage kt+2 are issued while stage kt is being multiplied: `s_waitcnt vmcnt(6)` retires
// exactly the oldest stage (6 LDS-DMA instructions per thread per stage: 4 for the 256-row A tile, 2
// for the 128-row W tile); never vmcnt(0) inside the loop.
constexpr int G2_BM = 256, G2_STAGE = (G2_BM + GBN) * GBK * 2;  // 48 KB

// Ping-pong schedule (the lock-step version of this tile -- one barrier per k-tile, lab/dvt_vit_lab.inc --
// ran the MFMA pipe 26-33 % busy: the two waves of a SIMD want the matrix pipe in the same window and
// both leave it idle while they stage / read the next tile).  Here every k-tile
// has a LOAD segment (issue the DMA of tile kt+2, read all fragments of tile kt into registers)
// and a COMPUTE segment (32 MFMAs), each closed by a barrier, and waves 4-7 ("group B") execute
// ONE extra barrier up front: for the whole loop group B is one segment behind group A, i.e. one
// group's MFMAs run beside the other group's DMA issue + ds_reads (the 8-phase idea of the CDNA
// guide, reduced to two phases).  Correctness of the hand-off: a wave waits for its own stage-
// (kt+1) DMA (`vmcnt(6)`) and its fragment reads (`lgkmcnt(0)`) at the END of LOAD(kt), so by the
// time any wave starts LOAD(kt+1) both groups have passed a barrier behind those waits; the DMA
// into buffer (kt+2) % 3 is issued one barrier after the last read of tile kt-1 by either group.
template <int EPI>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_bf16_kernel_pp(GemmBArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[3 * G2_STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const bool group_b = wave >= 4;
  const TileMap tm = map_tile(blockIdx.x, gridDim.x, p.M / G2_BM, p.N / GBN, p.group);
  const int m0 = tm.m * G2_BM, n0 = tm.n * GBN;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nk = p.K / GBK;
  const bf16_t* srcA[4];
  const bf16_t* srcW[2];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int s_ = it * 512 + tid, row = s_ >> 3, c = (s_ & 7) ^ (row & 7);
    srcA[it] = p.A + (size_t)(m0 + row) * p.K + c * 8;
    if (it < 2) srcW[it] = p.W + (size_t)(n0 + row) * p.K + c * 8;
  }
  const int ldsw = wave * 1024;
#define PP_ISSUE(kt)                                                                  \
  do {                                                                                \
    char* st_ = smem + ((kt) % 3) * G2_STAGE + ldsw;                                  \
    const int ko_ = (kt) * GBK;                                                       \
    _Pragma("unroll") for (int it = 0; it < 4; ++it)                                  \
        glds16(srcA[it] + ko_, st_ + it * 8192);                                      \
    _Pragma("unroll") for (int it = 0; it < 2; ++it)                                  \
        glds16(srcW[it] + ko_, st_ + G2_BM * GBK * 2 + it * 8192);                    \
  } while (0)
  PP_ISSUE(0);
  if (nk > 1) {
    PP_ISSUE(1);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();           // tile 0 is in LDS for everybody
  if (group_b) __builtin_amdgcn_s_barrier();  // group B: one segment behind from here on
  const int rowa = wm * 64 + (lane & 15), rowb = wn * 64 + (lane & 15), cg = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    // ---------------- LOAD segment ----------------
    if (kt + 2 < nk) PP_ISSUE(kt + 2);
    const char* As = smem + (kt % 3) * G2_STAGE;
    const char* Bs = As + G2_BM * GBK * 2;
    bf16x8 a0[4], b0[4], a1[4], b1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a0[i] = read_frag(As, rowa + i * 16, cg);
#pragma unroll
    for (int j = 0; j < 4; ++j) b0[j] = read_frag(Bs, rowb + j * 16, cg);
#pragma unroll
    for (int i = 0; i < 4; ++i) a1[i] = read_frag(As, rowa + i * 16, 4 + cg);
#pragma unroll
    for (int j = 0; j < 4; ++j) b1[j] = read_frag(Bs, rowb + j * 16, 4 + cg);
    if (kt + 2 < nk)
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");  // own DMA of tile kt+1 has landed
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // fragments are in registers
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    // ---------------- COMPUTE segment ----------------
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[i], b0[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[i], b1[j], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }
#undef PP_ISSUE
  if (!group_b) __builtin_amdgcn_s_barrier();  // group A: balance group B's extra barrier
  __syncthreads();  // every wave is done with the operand stages: the buffers become epilogue space
  gemm_epilogue_lds<EPI>(p, acc, m0, n0, wm, wn, wave, lane, smem);
}

// ---- 256x256x64 tile, 8-phase schedule ("8p") ------------------------------------------------
// A two-stage ring of whole 64-KB k-tiles (lab/dvt_vit_lab.inc, `sq`) drains its LDS-DMA queue at a
// __syncthreads per k-tile, so every k-tile costs one loaded L2 latency (~1.7 us against 0.85 us of
// MFMA work).  Here the 64-KB k-tile is
// split into four 16-KB HALF-TILES (A0, A1, B0, B1: 128 operand rows x 64 k each) that are
// consumed and re-staged one per phase, so four half-tiles (64 KB per CU) are in flight at ALL
// times and nothing ever waits for vmcnt(0).  (A ten-slot ring over the whole 160-KB LDS with six
// half-tiles in flight measured the same rate -- the k-loop is not bytes-in-flight bound -- and
// would evict the co-resident fit kernels, so the ring stays at eight slots.)
//   half h of A holds rows m0 + (r>>6)*128 + h*64 + (r&63), half h of W rows n0 + (r>>5)*64 +
//   h*32 + (r&31) (r = local row): wave (wm, wn) still owns the contiguous 128 x 64 output block.
//   phase   ds_read (-> regs)   MFMA quadrant     LDS-DMA issued        s_waitcnt (end of L)
//   P1(t)   B0(t), A0(t)        (A0, B0)          B1(t+1)               vmcnt(8)  [B1(t) landed]
//   P2(t)   B1(t)               (A0, B1)          A1(t+1)               vmcnt(8)  [A1(t)]
//   P3(t)   A1(t)               (A1, B1)          A0(t+2)               --
//   P4(t)   --                  (A1, B0)          B0(t+2)               vmcnt(8)  [A0, B0 (t+1)]
// Every phase is {L: ds_reads + DMA issue + counted wait} barrier {M: 16 MFMAs} barrier; the
// waves with wm == 1 run half a phase behind (one extra barrier up front), so on each SIMD one
// wave is in its MFMA segment while the other one issues loads.  Hazards:
//   WAR  a half-tile is re-staged two phases after the phase that read it: all reads of phase p
//        (both groups) have retired at the second barrier of phase p.
//   RAW  a half-tile is read one phase after the phase whose L segment waited for it: the waits
//        of both groups precede the second barrier of that phase.
template <int MODE>  // 0 steady state, 1 tile nk-2 (no issue in P3/P4), 2 tile nk-1 (no issue)
struct P8Wait;
template <> struct P8Wait<0> { static constexpr int w1 = 8, w2 = 8, w4 = 8; };
template <> struct P8Wait<1> { static constexpr int w1 = 8, w2 = 8, w4 = 4; };
template <> struct P8Wait<2> { static constexpr int w1 = 2, w2 = 0, w4 = -1; };

template <int N>
__device__ __forceinline__ void wait_vm() {
  if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

#define P8_BAR()                         \
  do {                                   \
    __builtin_amdgcn_sched_barrier(0);   \
    __builtin_amdgcn_s_barrier();        \
    __builtin_amdgcn_sched_barrier(0);   \
  } while (0)
#define P8_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
// 16 MFMAs: 4 m-frags x 2 n-frags x 2 k-steps; dependent pairs are 8 issues apart
#define P8_MFMA(IB, JB, AF, BF)                                                                   \
  do {                                                                                            \
    __builtin_amdgcn_s_setprio(1);                                                                \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                              \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                 \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                 \
        acc[IB + i][JB + j] =                                                                     \
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(AF[i][ks], BF[j][ks], acc[IB + i][JB + j], 0, 0, 0); \
    __builtin_amdgcn_s_setprio(0);                                                                \
  } while (0)

// ---- round 6: the walk of the ring ("8b").  The table above is round 5's walk (12 / 4 / 8 / 0 fragment reads per phase, ring
// parity a run-time value); it lives on in lab/dvt_vit_gemm8p_lab.inc as the developer library's schedule 13, bit-identical to
// this one (tests/test_gpu_lab.py).  Round 4's per-barrier stamps (profiles/r04/r04w_*) showed seven of a k-tile's eight
// half-phases at 325-345 cycles -- the partner group's 16 MFMAs + two barriers -- and the eighth, the load segment of P1, at
// 570-590: it carried 12 of the k-tile's 24 ds_read_b128 (B0 and A0) behind the k-tile boundary's address arithmetic (VALU:
// the parity offset of 12 read addresses and four 64-bit DMA source pointers), while P4's load segment read nothing.  Now:
//   * the k-loop is unrolled by two, so the parity of every slot is a literal: fragment-read addresses are loop-invariant
//     registers + instruction offsets, the DMA goes through two buffer descriptors (SGPRs) with one 32-bit lane offset per pass
//     and the half / k-tile in the scalar offset -- no VALU instruction in any load segment;
//   * B0 of k-tile t+1 is read in the load segment of P4(t), into the B registers that died with P3's MFMAs: the phases read
//     8 / 4 / 8 / 4 fragments (A0 | B1 | A1 | B0'), and the two B register sets swap roles every k-tile (hence the unroll);
//   * B0 is therefore needed one phase earlier: the stages are issued in the order B1(t+1) A1(t+1) B0(t+2) A0(t+2), one per
//     phase, and EVERY phase waits vmcnt(8) (four stages in flight, as before).
//   phase   ds_read (-> regs)    MFMA quadrant    LDS-DMA issued   s_waitcnt vmcnt(8) retires
//   P1(t)   A0(t)                (A0, B0)         B1(t+1)          B1(t)
//   P2(t)   B1(t)    -> bx       (A0, B1)         A1(t+1)          A1(t)
//   P3(t)   A1(t)                (A1, B1)         B0(t+2)          B0(t+1)
//   P4(t)   B0(t+1)  -> bx       (A1, B0)         A0(t+2)          A0(t+1)
// Hazards: a slot is re-staged three phases after the phase that read it (round 5: two); a half-tile is read one phase after
// the phase whose load segment waited for it; the waits of both groups precede the second barrier of that phase.
// Measured (profiles/r06/r06b_*, 398 views, random operands, interleaved with round 5's walk): qkv -0.6 %, proj -0.7 %,
// fc1 -1.7 %, fc2 (48 k-tiles: the k-loop itself) -3.4 %.  Issuing the stage inside the MFMA segment instead ("8m"
// placement on this walk) LOSES 1-7 %.  K / 64 must be even (launch_gemm).
// MODE of a k-tile: 0 steady state; 1 k-tile nk-2 (nothing to issue in P3 / P4); 2 k-tile nk-1 (nothing to issue).  The
// persistent kernel (gemm_bf16_kernel_8t) adds 3 = k-tile 0 of a tile whose k-tile 0 was staged under the previous tile
// (P1 / P2 need no wait) and 4 = k-tile nk-1 staging k-tile 0 of the NEXT tile, one half-tile per phase (rsAn / rsBn).
template <int MODE>
struct P8BWait;
template <> struct P8BWait<0> { static constexpr int w1 = 8, w2 = 8, w3 = 8, w4 = 8; };
template <> struct P8BWait<1> { static constexpr int w1 = 8, w2 = 8, w3 = 6, w4 = 4; };
template <> struct P8BWait<2> { static constexpr int w1 = 2, w2 = 0, w3 = -1, w4 = -1; };
template <> struct P8BWait<3> { static constexpr int w1 = -1, w2 = -1, w3 = 8, w4 = 8; };
template <> struct P8BWait<4> { static constexpr int w1 = 4, w2 = 4, w3 = -1, w4 = -1; };

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// Per-lane constants of the 8p / 8t k-loop (declares locals in the caller's scope): the DMA goes through two buffer
// descriptors (SGPRs) based at the tile's A / W rows -- per lane ONE 32-bit byte offset per pass (512 threads x 16 B = 64
// rows of a half-tile), the half (h) and the k-tile in the scalar offset: no 64-bit VALU address arithmetic in the load
// segments, 4 address registers instead of 16.  Fragment read offsets inside a half-tile: row*128 + ((ks*4 + cg) ^ (row & 7))*16;
// the same four offsets into the ring's second parity are registers of their own (opaque to the compiler): ds_read's
// instruction offset is 16 bits, the ring 128 KB -- left alone hipcc forms one address register per READ of parity 1 (12).
#define P8_LANE_SETUP()                                                                                                  \
  int voA[2], voB[2];                                                                                                    \
  _Pragma("unroll") for (int it = 0; it < 2; ++it) {                                                                     \
    const int s_ = it * 512 + tid, r = s_ >> 3, c = (s_ & 7) ^ (r & 7);                                                  \
    voA[it] = (((r >> 6) * 128 + (r & 63)) * p.lda + c * 8) * 2;                                                         \
    voB[it] = (((r >> 5) * 64 + (r & 31)) * p.ldw + c * 8) * 2;                                                          \
  }                                                                                                                      \
  const int hA = 64 * p.lda * 2, hB = 32 * p.ldw * 2; /* second half-tile: +64 A rows / +32 W rows */                    \
  constexpr int OFF_A0 = 0, OFF_A1 = 16384, OFF_B0 = 32768, OFF_B1 = 49152, BUF = 65536;                                 \
  char* const ldsw = smem + wave * 1024;                                                                                 \
  const int cg = lane >> 4;                                                                                              \
  const int ra = wm * 64 + (lane & 15), rb = wn * 32 + (lane & 15);                                                      \
  const int oa0 = ra * 128 + (((0 + cg) ^ (ra & 7)) << 4), oa1 = ra * 128 + (((4 + cg) ^ (ra & 7)) << 4);                \
  const int ob0 = rb * 128 + (((0 + cg) ^ (rb & 7)) << 4), ob1 = rb * 128 + (((4 + cg) ^ (rb & 7)) << 4);                \
  int oa0q = oa0 + 65536, oa1q = oa1 + 65536, ob0q = ob0 + 65536, ob1q = ob1 + 65536;                                    \
  asm volatile("" : "+v"(oa0q), "+v"(oa1q), "+v"(ob0q), "+v"(ob1q))
#define P8_RSRC(ptr, len) __builtin_amdgcn_make_buffer_rsrc((void*)(ptr), 0, (len), 0x00020000)
// stage half H (0 / 1) of operand X (A / B) of k-tile kt through descriptor RS into the slot at byte offset off
// (P8_AUX_A / P8_AUX_B: cache-policy bits of the two operand streams -- 0 in the product; the developer library's schedules
// 14 / 15 / 16 set nt (2) on A / W / both: profiles/r06/r06m_*)
#define P8_STAGE_RS(RS, X, H, kt, off)                                                                                   \
  do {                                                                                                                   \
    const int so_ = (kt) * (GBK * 2) + (H) * h##X;                                                                       \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(RS, (lds_ptr_t)(ldsw + (off)), 16, vo##X[0], so_, 0, P8_AUX_##X);           \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(RS, (lds_ptr_t)(ldsw + (off) + 8192), 16, vo##X[1], so_, 0, P8_AUX_##X);    \
  } while (0)
#define P8_STAGE(X, H, kt, off) P8_STAGE_RS(rs##X, X, H, kt, off)
#define P8_RD(base, off) (*reinterpret_cast<const bf16x8*>((base) + (off)))
// k-tile t of parity PAR (a literal); BC: the B registers that hold B0(t), BX: the other set
#define P8B_TILE(MODE, PAR, t, BC, BX)                                                            \
  do {                                                                                            \
    constexpr int bo_ = (PAR) * BUF, bn_ = bo_ ^ BUF;                                             \
    constexpr bool st12_ = MODE == 0 || MODE == 1 || MODE == 3, st34_ = MODE == 0 || MODE == 3;   \
    const int ra0_ = (PAR) ? oa0q : oa0, ra1_ = (PAR) ? oa1q : oa1;  /* this parity's A reads */   \
    const int rb0_ = (PAR) ? ob0q : ob0, rb1_ = (PAR) ? ob1q : ob1;  /* ... B reads */             \
    const int rn0_ = (PAR) ? ob0 : ob0q, rn1_ = (PAR) ? ob1 : ob1q;  /* the other parity's B0 */   \
    /* P1 */                                                                                      \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                               \
      a[i][0] = P8_RD(smem + OFF_A0 + i * 2048, ra0_);                                            \
      a[i][1] = P8_RD(smem + OFF_A0 + i * 2048, ra1_);                                            \
    }                                                                                             \
    if (st12_) P8_STAGE(B, 1, (t) + 1, bn_ + OFF_B1);                                             \
    if (MODE == 4) P8_STAGE_RS(rsBn, B, 0, 0, OFF_B0);                                            \
    wait_vm<P8BWait<MODE>::w1>();                                                                 \
    P8_BAR();                                                                                     \
    P8_LGKM0();                                                                                   \
    P8_MFMA(0, 0, a, BC);                                                                         \
    P8_BAR();                                                                                     \
    /* P2 */                                                                                      \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                               \
      BX[j][0] = P8_RD(smem + OFF_B1 + j * 2048, rb0_);                                           \
      BX[j][1] = P8_RD(smem + OFF_B1 + j * 2048, rb1_);                                           \
    }                                                                                             \
    if (st12_) P8_STAGE(A, 1, (t) + 1, bn_ + OFF_A1);                                             \
    if (MODE == 4) P8_STAGE_RS(rsAn, A, 0, 0, OFF_A0);                                            \
    wait_vm<P8BWait<MODE>::w2>();                                                                 \
    P8_BAR();                                                                                     \
    P8_LGKM0();                                                                                   \
    P8_MFMA(0, 2, a, BX);                                                                         \
    P8_BAR();                                                                                     \
    /* P3 */                                                                                      \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                               \
      a[i][0] = P8_RD(smem + OFF_A1 + i * 2048, ra0_);                                            \
      a[i][1] = P8_RD(smem + OFF_A1 + i * 2048, ra1_);                                            \
    }                                                                                             \
    if (st34_) P8_STAGE(B, 0, (t) + 2, bo_ + OFF_B0);                                             \
    if (MODE == 4) P8_STAGE_RS(rsBn, B, 1, 0, OFF_B1);                                            \
    wait_vm<P8BWait<MODE>::w3>();                                                                 \
    P8_BAR();                                                                                     \
    P8_LGKM0();                                                                                   \
    P8_MFMA(4, 2, a, BX);                                                                         \
    P8_BAR();                                                                                     \
    /* P4: B0 of the NEXT k-tile -> BX (dead: P3's MFMAs have been issued) */                      \
    if (MODE != 2 && MODE != 4) {                                                                 \
      _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                             \
        BX[j][0] = P8_RD(smem + OFF_B0 + j * 2048, rn0_);                                         \
        BX[j][1] = P8_RD(smem + OFF_B0 + j * 2048, rn1_);                                         \
      }                                                                                           \
    }                                                                                             \
    if (st34_) P8_STAGE(A, 0, (t) + 2, bo_ + OFF_A0);                                             \
    if (MODE == 4) P8_STAGE_RS(rsAn, A, 1, 0, OFF_A1);                                            \
    wait_vm<P8BWait<MODE>::w4>();                                                                 \
    P8_BAR();                                                                                     \
    P8_MFMA(4, 0, a, BC);                                                                         \
    P8_BAR();                                                                                     \
  } while (0)

// STAMP (developer library only, schedule 12): the tile's anatomy in WALL time -- s_memrealtime (100 MHz, not the shader clock:
// independent of DVFS) at kernel entry, at the first MFMA (prologue done), behind the k-loop, behind the last store's issue and
// behind its retirement, + HW_ID / XCC_ID (which CU): 8 u32 per workgroup at p.dbg (tools/lab_gemm8p_anatomy.py).
// KPOL: the cache policies that need an instruction form of their own (kpol_of; 0 = the kernel of rounds 5-6 unchanged): 1 nt
// residual loads, 2 nt residual stores, 8 those stores sc1 instead, 4 nt xb stores (st_part stays plain, see gemm_epilogue_resid_sq), 16 sc1 `out` stores.  The nt
// hint on the bf16 outputs stays the run-time GemmBArgs::nt_store.
template <int EPI, bool STAMP = false, int AUX = 0, int KPOL = 0>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_bf16_kernel_8p(GemmBArgs p) {
  constexpr int P8_AUX_A = (AUX & 1) ? 2 : 0, P8_AUX_B = (AUX & 2) ? 2 : 0;  // nt on the A / W stream (lab schedules 14..16)
  __shared__ __attribute__((aligned(16))) char smem[8 * EP_WAVE_BYTES];  // 136 KB >= 8 half-tiles (128 KB)
  unsigned long long ts_[5] = {0, 0, 0, 0, 0};
  if constexpr (STAMP) ts_[0] = __builtin_amdgcn_s_memrealtime();
  // De-synchronised start (dvt_tune_set(1, -700 - pct); round 5: null except proj, default off): the workgroups of the first
  // round wait a hash-spread fraction of one tile time (s_memrealtime, 100 MHz).  Results do not depend on it.
  if (p.stagger_ticks > 0 && blockIdx.x < 256) {
    const unsigned h_ = ((unsigned)blockIdx.x * 2654435761u) >> 16;  // 16-bit hash of the block id
    const unsigned long long wait_ = ((unsigned long long)p.stagger_ticks * h_) >> 16;
    const unsigned long long t0_ = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0_ < wait_) __builtin_amdgcn_s_sleep(16);
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const TileMap tm = map_tile_fast(p.ord, blockIdx.x, gridDim.x, p.M >> 8, p.N >> 8);
  // XCD-column order: a slot beyond this XCD's rectangle has no tile and the workgroup ends here (workgroup-uniform, before
  // any barrier or memory access; the hardware drains the scalar loads first).  Written as the instruction, not as `return`:
  // the second exit block costs the GELU and residual instantiations 4 VGPRs (236 / 234 against 232 / 230), the budget that
  // lets a wave of the fit's streaming kernels share the SIMD
  // INVARIANT: the compiler believes control goes on with m0 = -256, so NOTHING that touches memory through tm / m0 / n0 --
  // the operand descriptors' LDS-DMA, the stagger loop excepted (it reads no tile) -- may move above this line.  The
  // "memory" clobber forbids it to the compiler; keep it, and keep the map call and this exit ahead of every load when
  // editing.  (Checked in the assembly of all instantiations: the exit precedes the first vector-memory / LDS instruction.)
  if (tm.m < 0) asm volatile("s_endpgm" ::: "memory");
  const int m0 = tm.m * 256, n0 = tm.n * 256;

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nk = p.K / GBK;  // even, >= 2 (launch_gemm checks)
  P8_LANE_SETUP();
  const __amdgpu_buffer_rsrc_t rsA = P8_RSRC(p.A + (size_t)m0 * p.lda, 0x7fffffff);
  const __amdgpu_buffer_rsrc_t rsB = P8_RSRC(p.W + (size_t)n0 * p.ldw, 0x7fffffff);
  const __amdgpu_buffer_rsrc_t rsAn = rsA, rsBn = rsB;  // (MODE 4 is the persistent kernel's: not instantiated here)

  // prologue: the whole k-tile 0 in the order it is needed, then what P3 / P4 of "k-tile -1" would have issued
  unsigned ts_setup_ = 0, ts_issued_ = 0;
  if constexpr (STAMP) {
    asm volatile("" : "+v"(voA[0]), "+v"(voB[0]), "+v"(oa0q));  // (the setup arithmetic is complete here, not sunk below)
    ts_setup_ = (unsigned)__builtin_amdgcn_s_memrealtime();
  }
  P8_STAGE(B, 0, 0, OFF_B0);
  P8_STAGE(A, 0, 0, OFF_A0);
  P8_STAGE(B, 1, 0, OFF_B1);
  P8_STAGE(A, 1, 0, OFF_A1);
  P8_STAGE(B, 0, 1, BUF + OFF_B0);
  P8_STAGE(A, 0, 1, BUF + OFF_A0);
  if constexpr (STAMP) ts_issued_ = (unsigned)__builtin_amdgcn_s_memrealtime();
  wait_vm<8>();  // B0(0), A0(0) have landed
  P8_BAR();
  if (wm == 1) P8_BAR();  // group 1: half a phase behind from here on

  bf16x8 a[4][2], be[2][2], bo[2][2];
  // "P4 of k-tile -1": B0(0) -> the even k-tiles' B0 registers
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    be[j][0] = P8_RD(smem + OFF_B0 + j * 2048, ob0);
    be[j][1] = P8_RD(smem + OFF_B0 + j * 2048, ob1);
  }
  if constexpr (STAMP) ts_[1] = __builtin_amdgcn_s_memrealtime();
  int t = 0;
  for (; t < nk - 2; t += 2) {
    P8B_TILE(0, 0, t, be, bo);
    P8B_TILE(0, 1, t + 1, bo, be);
  }
  P8B_TILE(1, 0, t, be, bo);
  P8B_TILE(2, 1, t + 1, bo, be);
  if (wm == 0) P8_BAR();  // balance group 1's extra barrier
  __syncthreads();        // operand buffers become epilogue space
  if constexpr (STAMP) ts_[2] = __builtin_amdgcn_s_memrealtime();
  NextTilePf pf_{nullptr, p.pf_next, 0u, 0u};
  if (p.pf_next > 0 && (int)blockIdx.x + 256 < (int)gridDim.x) {
    const TileMap tn = map_tile_fast(p.ord, blockIdx.x + 256, gridDim.x, p.M >> 8, p.N >> 8);
    if (tn.m >= 0) pf_.src = tid < 256 ? p.A + (size_t)(tn.m * 256 + tid) * p.lda : p.W + (size_t)(tn.n * 256 + tid - 256) * p.ldw;
  }
  if constexpr (EPI == EPI_RESID) {
    gemm_epilogue_resid_sq<(KPOL & 1) ? 2 : 0, (KPOL & 2) ? ((KPOL & 8) ? 16 : 2) : 0, (KPOL & 4) != 0>(
        p, acc, m0 + wm * 128, n0 + wn * 64, wave, lane, smem, &pf_);
  } else {
    f32x4(&lo)[4][4] = *reinterpret_cast<f32x4(*)[4][4]>(&acc[0]);
    f32x4(&hi)[4][4] = *reinterpret_cast<f32x4(*)[4][4]>(&acc[4]);
    gemm_epilogue_lds<EPI, 4, (KPOL & 16) != 0>(p, lo, m0 + wm * 128, n0 + wn * 64, 0, 0, wave, lane, smem);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    gemm_epilogue_lds<EPI, 4, (KPOL & 16) != 0>(p, hi, m0 + wm * 128 + 64, n0 + wn * 64, 0, 0, wave, lane, smem, nullptr, &pf_);
  }
  pf_retire(pf_);
  if constexpr (STAMP) {
    ts_[3] = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ts_[4] = __builtin_amdgcn_s_memrealtime();
    if (p.dbg != nullptr && tid == 0) {  // wave 0 (group 0); one record per workgroup
      unsigned* d_ = p.dbg + (size_t)blockIdx.x * 8;
#pragma unroll
      for (int i = 0; i < 5; ++i) d_[i] = (unsigned)ts_[i];
      d_[5] = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_REG_HW_ID: wave / simd / cu / sh / se
      d_[6] = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // HW_REG_XCC_ID
      d_[7] = ((ts_setup_ - (unsigned)ts_[0]) & 0xffffu) | ((ts_issued_ - (unsigned)ts_[0]) << 16);  // setup done / 12 DMAs issued, ticks after entry
    }
  }
}

#ifdef DVT_LAB
#include "lab/dvt_vit_gemm8t.inc"  // "8t": this kernel as a persistent workgroup with an overlapped tile boundary (round 6, negative)
#endif
#undef P8B_TILE
#undef P8_STAGE
#undef P8_STAGE_RS
#undef P8_RSRC
#undef P8_RD
#undef P8_LANE_SETUP

// (Rounds 3 / 4 built two persistent variants of this kernel -- "8q": register epilogue + tile loop, removed; "4w": four
// waves, deferred epilogue, lab/dvt_vit_gemm4w.inc -- neither beat it: profiles/LOG.md 5 finding 3, profiles/r04/README.md.)
#ifdef DVT_LAB
typedef const __attribute__((address_space(4))) GemmBArgs* kernarg_ptr_t;

#include "lab/dvt_vit_gemm4w.inc"
#include "lab/dvt_vit_gemm8p_lab.inc"
#include "lab/dvt_vit_lab.inc"
#endif

// W bytes kept L2-resident per N-tile group.  4800 KiB = every N tile of a K = 768 GEMM in ONE group (qkv: 9
// tiles, fc1: 12): each 393-KB A panel is then fetched once instead of once per group (measured: GEMMs 907 ->
// 931 TF/s in the extractor; 9600 KiB the same, 1200 KiB 900).  Round 7, current kernel, 396 views: 1200 / 2400 / 4800 KiB
// within +-1 % of each other on qkv and fc1 (profiles/r07/): the group budget no longer moves a launch.
int g_vit_group_bytes = 4800 * 1024;
// M panels per block of the tile order, 0 = auto (launch_gemm): on the swept launches (the four GEMMs of a bf16 ViT-B block,
// >= 256 M panels) qkv 8, fc1 4, proj / fc2 2; elsewhere 4 when a group has >= 6 N tiles, else 1, as before.  Round 7 at 396 views (profiles/r07/r07k_*): qkv 4 -> 8 or 16 +6-8 %
// (32: +1 %, 64: -5 %); fc1 flat from 2 to 16, 1 and 32 lose 2-7 %; proj 1 -> 2 or 4 +4-7 %, fc2 1 -> 2 +1 %, 8 and 16 lose.
// Rounds 2-6 (4 / 1), measured with the round-2 kernel at 128 views:
// PMC FETCH_SIZE per launch, 128 views (profiles/r02/pmc_vit/): qkv 1.57 -> 1.10 GB, fc1 1.65 -> 1.39 GB with
// blocks of 4; the N = 768 GEMMs (3 N tiles) get WORSE with blocks (1.53 -> 1.68 GB) and keep n-fastest.
// Time moves by +1 % only (919 -> 930 TF/s): the L2 misses are served by the memory-side cache.
int g_vit_mblock = 0;
// bf16 output stores with the non-temporal hint: measured no effect on time or FETCH_SIZE (kept as a knob)
int g_vit_nt_store = 0;
// XCD column sets of the 8p kernel's tile order (dvt_tile_map.h): 0 = auto (g_vit_xcols_bytes), 1 / 2 / 4 forced where it
// divides the N tile count (dvt_tune_set(1, -70 - xcols)).
int g_vit_xcols = 0;
// auto: the smallest xcols that leaves one XCD at most this many bytes of W (dvt_tune_set(1, -100000 - KiB)); 0 = never
// split (the order of rounds 2-6).  2400 KiB: fc1 at dim 768 (12 slabs of 384 KiB) runs as 2 column sets of 6.
int g_vit_xcols_bytes = 2400 * 1024;
// EPOL_* mask (dvt_tune_set(1, -200000 - mask)): streaming cache policy on the epilogues' once-touched traffic, 0 = none;
// -200000 - 128 = auto
int g_vit_epi_policy = -1;  // -1 = auto: EPOL_DEFAULT on the swept launches (launch_gemm), none elsewhere
// dvt_tune_set(1, -700 - pct): the first round of 8p workgroups starts spread over pct % of the modelled tile time (k-loop
// 1.68 us per k-tile + epilogue); 0 = all together
int g_vit_stagger_pct = 0;
int g_vit_pf_next = 0;  // dvt_tune_set(1, -570 - n): GemmBArgs::pf_next (0 = off, the default: measured null, profiles/r06/r07a_*)

}  // namespace

template <int EPI>
int launch_gemm(const GemmArgs& a0, hipStream_t s) {
  if (a0.M % GBM || a0.N % GBN || a0.K % GBK || a0.M <= 0) return DVT_E_BADARG;
  if (IS_X3(EPI) && a0.M % 256) return DVT_E_BADARG;  // written for the LDS-staged epilogues (256-row tiles) only
  GemmBArgs a{a0};
  if (!a.lda) a.lda = a.K;
  if (!a.ldw) a.ldw = a.K;
  a.dim_ok_sq = (!IS_QKV(EPI)) || (a.dim % 256 == 0);
  // V^T: vt_rows real rows of whole images, a multiple of 8 (the LDS-staged epilogue's 8-token chunks)
  if (IS_QKV(EPI) && (a.s_pad <= 0 || a.s_pad % 8 || a.vt_rows <= 0 || a.vt_rows % a.s_pad || a.vt_rows > a.M))
    return DVT_E_BADARG;
  bool sq = g_vit_gemm_variant >= 4;  // (lab: 5..12 are variants of the same tile)
#ifdef DVT_LAB
  sq = sq || g_vit_gemm_variant == 0;
#endif
  sq = sq && a.M % 256 == 0 && a.N % 256 == 0 && a.dim_ok_sq && a.K >= 2 * GBK && (a.K / GBK) % 2 == 0;  // (8p: k-tiles in pairs)
  // The folded LayerNorm's consumer side (ln_stats) lives in the LDS-staged epilogues (256-row tiles), its producer side (xb /
  // st_part) in the 256 x 256 residual epilogue: a launch that would take another kernel is refused, not silently unfolded
  if (a.ln_stats != nullptr && !(sq || (a.M % G2_BM == 0 && g_vit_gemm_variant != 1))) return DVT_E_BADARG;
  if ((a.xb != nullptr || a.st_part != nullptr) && !(sq && EPI == EPI_RESID && a.xb != nullptr && a.st_part != nullptr))
    return DVT_E_BADARG;
  {
    const int nt = a.N / GBN;
    int g = g_vit_group_bytes / (GBN * a.K * 2);
    g = g < 1 ? 1 : (g > nt ? nt : g);
    while (g > 1 && nt % g) --g;  // prefer a divisor of the tile count (equal groups)
    a.group = g;
  }
  DvtProbeScope probe(DVT_PROBE_VIT_GEMM, s, a.work > 0.0 ? a.work : 2.0 * a.M * a.N * a.K);
  if (sq) {
    const int nt = a.N / 256;
    // N tiles per group: W slices of a group stay L2-resident, but never fewer than 3 tiles share
    // an A panel (K = 3072: one tile per group re-read A three times from HBM, 1.03 -> 1.23 PF/s)
    int g = g_vit_group_bytes / (256 * a.K * 2);
    g = g < 3 ? 3 : g;
    g = g > nt ? nt : g;
    while (g > 1 && nt % g) --g;
    a.group = g;
    // The round-7 defaults (M blocks, column sets, epilogue policy) hold for the launches they were measured on and for no
    // other: the four GEMMs of a bf16 ViT-B block (qkv, fc1, proj, fc2 by epilogue AND shape) at >= 256 M panels, i.e. many
    // rounds of 256 tiles (swept at 2005 and 2129 panels, profiles/r07/).  Everything else -- the patch embedding, SwiGLU,
    // ViT-L / ViT-g, the fp32 extractor's bf16x3 launches (EPI_F32, EPI_*_X3, and its EPI_RESID at K = 3 dim), short launches
    // -- keeps the order, the M blocks and the plain stores of rounds 2-6 unless a tune key says otherwise.
    const bool swept = a.M / 256 >= 256 && ((EPI == EPI_QKV && a.N == 2304 && a.K == 768) || (EPI == EPI_GELU && a.N == 3072 && a.K == 768) ||
                                            (EPI == EPI_RESID && a.N == 768 && (a.K == 768 || a.K == 3072)));
    // M panels per block, auto (g_vit_mblock): rounds 2-6: 4 where a group has >= 6 N tiles, else 1.  Swept: qkv 8, fc1 4,
    // proj / fc2 2
    int mb_auto = g >= 6 ? 4 : 1;
    if (swept) mb_auto = EPI == EPI_QKV ? 8 : (EPI == EPI_GELU ? 4 : 2);
    a.mblock = g_vit_mblock > 0 ? g_vit_mblock : mb_auto;
    // epilogue cache policy of this launch's outputs: a mask set by tune key holds for every launch but the X3 epilogues
    // (the fp32 extractor's own), the default for the swept ones
    const int epol = IS_X3(EPI) ? 0 : (g_vit_epi_policy >= 0 ? g_vit_epi_policy : (swept ? EPOL_DEFAULT : 0));
    a.nt_store = (epol & (IS_QKV(EPI) ? EPOL_QKV_ST : EPOL_HID_ST)) ? 1 : g_vit_nt_store;
    const dim3 grid8((a.M / 256) * nt);
    a.ord = tile_order_make(a.M / 256, nt, a.group, a.mblock, 1);  // (every kernel but the product 8p walks xcols = 1)
    if (g_vit_stagger_pct > 0 && grid8.x > 512) {  // (a launch of fewer than two rounds has nothing to de-synchronise)
      // (EPI_SWIGLU borrows the GELU epilogue's measured 10.5 us: its own has not been measured)
      const double epi_us = EPI == EPI_RESID ? 20.0 : ((IS_GELU(EPI) || EPI == EPI_SWIGLU) ? 10.5 : 5.6);
      const double tile_us = 1.68 * (a.K / GBK) + epi_us;
      a.stagger_ticks = (int)(tile_us * 100.0 * g_vit_stagger_pct / 100.0);
    }
    a.pf_next = g_vit_pf_next;
#ifdef DVT_LAB
    if (int rc = 0; lab_launch_gemm<EPI>(a, s, grid8, nt, &rc)) return rc;  // (lab/dvt_vit_lab.inc: a selected lab kernel took it)
#endif
    // XCD column sets (dvt_tile_map.h): g_vit_xcols, or with 0 (auto) the smaller of {1, 2} that divides nt and leaves an
    // XCD at most g_vit_xcols_bytes of W; 1 (the grouped order) where neither does.  Four column sets are never chosen
    // here: at the one shape where they were measured (fc1, dim 768) they lose 2-3 % (profiles/r07/README.md).  Auto splits
    // swept launches only (many rounds: the rectangles differ by up to `group` tiles per XCD, which a launch of about one
    // round would pay as a whole extra round); a forced xcols holds for every launch but the X3 epilogues.
    int xcols = 1;
    if (!IS_X3(EPI)) {
      if (g_vit_xcols > 0) xcols = g_vit_xcols;
      else if (g_vit_xcols_bytes > 0 && swept)
        for (int xc = 1; xc <= 2; xc *= 2)
          if (nt % xc == 0 && (long long)(nt / xc) * 256 * a.K * 2 <= g_vit_xcols_bytes) {
            xcols = xc;
            break;
          }
    }
    if (tile_order_xcols(nt, xcols) > 1) a.ord = tile_order_make(a.M / 256, nt, a.group, a.mblock, xcols);
    const dim3 gridx(tile_order_grid(a.ord, a.M / 256, nt));
    // policies that are an instruction form (gemm_bf16_kernel_8p's KPOL): the residual stream's -- one of its three bits, or
    // all of them (vit_gemm_tune admits nothing else) -- and the write-through `out` stores of the bias / GELU epilogues
#define LAUNCH_8P(KP) hipLaunchKernelGGL((gemm_bf16_kernel_8p<EPI, false, 0, KP>), gridx, dim3(512), 0, s, a)
    bool launched = false;
    if constexpr (EPI == EPI_RESID) {
      const int sc1 = (epol & EPOL_RESID_SC1) ? 8 : 0;
      launched = true;
      switch ((epol & 7) | ((epol & EPOL_RESID_ST) ? sc1 : 0)) {
        case 1: LAUNCH_8P(1); break;
        case 2: LAUNCH_8P(2); break;
        case 2 | 8: LAUNCH_8P(2 | 8); break;
        case 4: LAUNCH_8P(4); break;
        case 7: LAUNCH_8P(7); break;
        case 7 | 8: LAUNCH_8P(7 | 8); break;
        default: launched = false;
      }
    } else if constexpr (EPI == EPI_BIAS || EPI == EPI_GELU) {
      if ((epol & EPOL_HID_ST) && (epol & EPOL_HID_SC1)) {
        LAUNCH_8P(16);
        launched = true;
      }
    }
    if (!launched) LAUNCH_8P(0);
#undef LAUNCH_8P
    DVT_CHECK_LAUNCH();
    return 0;
  }
  if (a.M % G2_BM == 0 && g_vit_gemm_variant != 1) {
    const int tiles = (a.M / G2_BM) * (a.N / GBN);
#ifdef DVT_LAB
    if (int rc = 0; lab_launch_gemm_256<EPI>(a, s, tiles, &rc)) return rc;  // (schedule 2, the lock-step kernel of this tile)
#endif
    hipLaunchKernelGGL((gemm_bf16_kernel_pp<EPI>), dim3(tiles), dim3(512), 0, s, a);
    DVT_CHECK_LAUNCH();
    return 0;
  }
  if (IS_X3(EPI)) return DVT_E_BADARG;  // the 128 x 128 kernel's register epilogue does not write the split outputs
  const int tiles = (a.M / GBM) * (a.N / GBN);
  hipLaunchKernelGGL((gemm_bf16_kernel<EPI>), dim3(tiles), dim3(256), 0, s, a);
  DVT_CHECK_LAUNCH();
  return 0;
}

// the nine epilogues: what the forward loops (dvt_vit.hip; dvt_vit_f32.hip through the entry points below) launch
template int launch_gemm<EPI_BIAS>(const GemmArgs&, hipStream_t);
template int launch_gemm<EPI_QKV>(const GemmArgs&, hipStream_t);
template int launch_gemm<EPI_GELU>(const GemmArgs&, hipStream_t);
template int launch_gemm<EPI_RESID>(const GemmArgs&, hipStream_t);
template int launch_gemm<EPI_EMBED>(const GemmArgs&, hipStream_t);
template int launch_gemm<EPI_F32>(const GemmArgs&, hipStream_t);
template int launch_gemm<EPI_GELU_X3>(const GemmArgs&, hipStream_t);
template int launch_gemm<EPI_QKV_X3>(const GemmArgs&, hipStream_t);
template int launch_gemm<EPI_SWIGLU>(const GemmArgs&, hipStream_t);

bool vit_gemm_sq_schedule() { return g_vit_gemm_variant >= 4; }

// The GEMM's share of dvt_tune_set(1, v) (dvt_vit_tune, dvt_vit.hip).  The product library accepts only values under which
// every entry point still computes its documented result (alternative schedules / orders that the GPU tests hold against the
// oracle); everything that selects a superseded kernel, an experiment or a timing build exists in lab builds (-DDVT_LAB) only
// (lab_gemm_tune) and is not known here.
int vit_gemm_tune(int v) {
  if (v == -50 || v == -51) {  // non-temporal bf16 output stores off / on
    g_vit_nt_store = v == -51;
    return 0;
  }
  if (v == -70 || v == -71 || v == -72 || v == -74) {  // 8p GEMM: XCD column sets of the tile order, -70 = auto
    g_vit_xcols = -70 - v;
    return 0;
  }
  if (v <= -100000 && v >= -100000 - 65536) {  // ... auto: W bytes per XCD (KiB) up to which a launch is not split further, 0 = never split
    g_vit_xcols_bytes = (-100000 - v) * 1024;
    return 0;
  }
  if (v == -200000 - 128) {  // ... auto (default)
    g_vit_epi_policy = -1;
    return 0;
  }
  if (v <= -200000 && v >= -200000 - EPOL_ALL) {  // streaming cache policy of the GEMM epilogues' once-touched traffic (EPOL_* mask)
    const int rs = (-200000 - v) & 7;  // the residual stream's three bits: one of them or all (the instantiated kernels)
    if (rs == 3 || rs == 5 || rs == 6) return DVT_E_BADARG;
    g_vit_epi_policy = -200000 - v;
    return 0;
  }
  if (v <= -570 && v >= -572) {  // 8p GEMM: L2 prefetch of the next workgroup's first 0 / 1 / 2 k-tiles (NextTilePf; results do not depend on it)
    g_vit_pf_next = -570 - v;
    return 0;
  }
#ifdef DVT_LAB
  if (const int rc = lab_gemm_tune(v); rc != VIT_TUNE_NOT_MINE) return rc;  // (the lab's keys and its wider set of schedules)
#endif
  if (v <= -700 && v >= -1100) {  // -700 - pct: de-synchronised start of the 8p workgroups (see the kernel), 0 = off
    g_vit_stagger_pct = -700 - v;
    return 0;
  }
  if (v <= -100 && v > -200) {  // -100 - b: M panels per block of the tile order
    g_vit_mblock = -100 - v;  // 0 = auto
    return 0;
  }
  if (v >= 16) {  // values >= 16: L2 group budget in KiB
    g_vit_group_bytes = v * 1024;
    return 0;
  }
  if (v != 1 && v != 3 && v != 4) return VIT_TUNE_NOT_MINE;  // the schedules the product library contains
  g_vit_gemm_variant = v;
  return 0;
}

// device buffer of the 8p timing builds (lab builds; the product library has none: DVT_E_BADARG)
extern "C" int dvt_vit_debug_buffer(void* dev_u32) {
#ifdef DVT_LAB
  if (lab_set_debug_buffer(dev_u32)) return 0;
#endif
  (void)dev_u32;
  return DVT_E_BADARG;
}

extern "C" int dvt_vit_gemm_bias(const void* x, const void* w, const float* b, void* y, int m,
                                 int n, int k, void* stream) {
  if (!x || !w || !y) return DVT_E_BADARG;
  GemmBArgs a{};
  a.A = (const bf16_t*)x; a.W = (const bf16_t*)w; a.M = m; a.N = n; a.K = k;
  a.bias = b; a.out = (bf16_t*)y;
  a.lda = a.ldw = k;
  return launch_gemm<EPI_BIAS>(a, (hipStream_t)stream);
}

// fc1-type GEMM as the extractor launches it: y (bf16) = [GELU]( rstd * (x . w'^T - mean * cs) + b' ) with the LayerNorm folded
// (ln_stats [m] (mean, rstd), ln_cs [n]; both null: y = [GELU](x . w^T + b))
extern "C" int dvt_vit_gemm_lnfold(const void* x, const void* w, const float* b, void* y, int m, int n, int k,
                                   const void* ln_stats, const float* ln_cs, int gelu, void* stream) {
  if (!x || !w || !y || (ln_stats == nullptr) != (ln_cs == nullptr)) return DVT_E_BADARG;
  GemmBArgs a{};
  a.A = (const bf16_t*)x; a.W = (const bf16_t*)w; a.M = m; a.N = n; a.K = k;
  a.bias = b; a.out = (bf16_t*)y;
  a.lda = a.ldw = k;
  a.ln_stats = (const float2*)ln_stats;
  a.ln_cs = ln_cs;
  if (gelu) return launch_gemm<EPI_GELU>(a, (hipStream_t)stream);
  if (ln_stats != nullptr) return DVT_E_BADARG;  // the bias epilogue has no folded form
  return launch_gemm<EPI_BIAS>(a, (hipStream_t)stream);
}

extern "C" int dvt_vit_swiglu_pack_index(int p, int n_hidden) {
  if (n_hidden <= 0 || n_hidden % 32 || p < 0 || p >= 2 * n_hidden) return -1;
  const int blk = p >> 6, q = p & 63;
  return q < 32 ? 32 * blk + q : n_hidden + 32 * blk + (q - 32);
}

// The SwiGLU fc1 GEMM as dvt_vit_forward launches it for ViT-g (EPI_SWIGLU): y [m, n_hidden] = silu(gate) * value from the
// PACKED [2 n_hidden, k] weights, optionally with the LayerNorm folded
extern "C" int dvt_vit_gemm_swiglu(const void* x, const void* w, const float* b, void* y, int m, int n_hidden, int k,
                                   const void* ln_stats, const float* ln_cs, void* stream) {
  if (!x || !w || !y || (ln_stats == nullptr) != (ln_cs == nullptr) || n_hidden <= 0 || n_hidden % 64) return DVT_E_BADARG;
  if (ln_stats != nullptr && b == nullptr) return DVT_E_BADARG;  // (the folded epilogue reads b' unconditionally)
  GemmBArgs a{};
  a.A = (const bf16_t*)x; a.W = (const bf16_t*)w; a.M = m; a.N = 2 * n_hidden; a.K = k;
  a.bias = b; a.out = (bf16_t*)y;
  a.lda = a.ldw = k;
  a.ln_stats = (const float2*)ln_stats;
  a.ln_cs = ln_cs;
  return launch_gemm<EPI_SWIGLU>(a, (hipStream_t)stream);
}

extern "C" int dvt_vit_gemm_residual(const void* a_in, const void* w, const float* b, const float* gamma,
                                     float* x, int m, int n, int k, void* stream) {
  if (!a_in || !w || !gamma || !x) return DVT_E_BADARG;
  GemmBArgs a{};
  a.A = (const bf16_t*)a_in; a.W = (const bf16_t*)w; a.M = m; a.N = n; a.K = k;
  a.bias = b; a.x = x; a.gamma = gamma;
  return launch_gemm<EPI_RESID>(a, (hipStream_t)stream);
}

extern "C" int dvt_vit_gemm_f32out(const void* a_in, const void* w, const float* b, float* y, int m, int n, int k,
                                   void* stream) {
  if (!a_in || !w || !y) return DVT_E_BADARG;
  GemmBArgs a{};
  a.A = (const bf16_t*)a_in; a.W = (const bf16_t*)w; a.M = m; a.N = n; a.K = k;
  a.bias = b; a.x = y;
  return launch_gemm<EPI_F32>(a, (hipStream_t)stream);
}

// The qkv GEMM exactly as dvt_vit_forward launches it (EPI_QKV): q | k into qk [m, 2 dim], V^T into vt [batch, heads, 64, s_pad]
extern "C" int dvt_vit_gemm_qkv(const void* x, const void* w, const float* b, void* qk, void* vt, int m, int dim, int heads,
                                int s_pad, int batch, const void* ln_stats, const float* ln_cs, float q_scale, void* stream) {
  if (!x || !w || !qk || !vt || batch <= 0 || heads <= 0 || dim != heads * 64 || s_pad <= 0 || s_pad % 32 ||
      (ln_stats == nullptr) != (ln_cs == nullptr))
    return DVT_E_BADARG;
  if ((long long)m != ((long long)batch * s_pad + 255) / 256 * 256) return DVT_E_BADARG;
  if (ln_stats != nullptr && (m % 256 || (3 * dim) % 256 || b == nullptr)) return DVT_E_BADARG;  // the forward's condition
  GemmBArgs a{};
  a.A = (const bf16_t*)x; a.W = (const bf16_t*)w; a.M = m; a.N = 3 * dim; a.K = dim;
  a.bias = b; a.out = (bf16_t*)qk; a.vt = (bf16_t*)vt;
  a.ln_stats = (const float2*)ln_stats; a.ln_cs = ln_cs;
  a.dim = dim; a.heads = heads; a.s_pad = s_pad; a.vt_rows = batch * s_pad;
  a.q_scale = q_scale;
  return launch_gemm<EPI_QKV>(a, (hipStream_t)stream);
}

// The proj / fc2 GEMM of the folded forward: the residual epilogue that also writes xb = bf16(x) and the per-row partial sums
// into part_scratch [n / 64][m] (float2), then ln_stats_finalize_kernel -> stats [m] (mean, rstd) of the new x
extern "C" int dvt_vit_gemm_residual_stats(const void* a_in, const void* w, const float* b, const float* gamma, float* x,
                                           void* xb, void* stats, void* part_scratch, int m, int n, int k, float eps,
                                           void* stream) {
  if (!a_in || !w || !gamma || !x || !xb || !stats || !part_scratch || m <= 0 || n <= 0) return DVT_E_BADARG;
  GemmBArgs a{};
  a.A = (const bf16_t*)a_in; a.W = (const bf16_t*)w; a.M = m; a.N = n; a.K = k;
  a.bias = b; a.x = x; a.gamma = gamma;
  a.xb = (bf16_t*)xb; a.st_part = (float2*)part_scratch;
  const int rc = launch_gemm<EPI_RESID>(a, (hipStream_t)stream);  // (DVT_E_BADARG unless the 256 x 256 kernel takes it)
  if (rc) return rc;
  return launch_ln_stats_finalize((const float2*)part_scratch, n / 64, m, 1.0f / (float)n, eps, (float2*)stats, (hipStream_t)stream);
}

// fc1 of the bf16x3 mode: out3 [m, 3 n] = split(GELU(a . w^T + b)) -- the next GEMM's A operand, no fp32 round trip
extern "C" int dvt_vit_gemm_gelu_x3(const void* a_in, const void* w, const float* b, void* out3, int m, int n, int k,
                                    void* stream) {
  if (!a_in || !w || !out3) return DVT_E_BADARG;
  GemmBArgs a{};
  a.A = (const bf16_t*)a_in; a.W = (const bf16_t*)w; a.M = m; a.N = n; a.K = k;
  a.bias = b; a.out = (bf16_t*)out3;
  return launch_gemm<EPI_GELU_X3>(a, (hipStream_t)stream);
}

// qkv of the bf16x3 mode: q | k as (hi, lo) [m, 2 dim] and V^T as (hi, lo) [batch, heads, 64, s_pad] in `scratch`
// (dvt_vit_attention_x3_scratch_bytes: the layout dvt_vit_attention_x3_presplit reads)
extern "C" int dvt_vit_gemm_qkv_x3(const void* a_in, const void* w, const float* b, void* scratch, int m, int dim, int heads,
                                   int s_pad, int batch, int k, void* stream) {
  // s_pad % 128: what its one consumer, dvt_vit_attention_x3_presplit, takes -- checked here, before anything is written
  if (!a_in || !w || !scratch || batch <= 0 || dim != heads * 64 || s_pad <= 0 || s_pad % 128) return DVT_E_BADARG;
  const X3Scratch L = x3_scratch(batch, heads, s_pad);
  if (m != L.m) return DVT_E_BADARG;  // whole 256-row tiles over batch * s_pad rows, exactly
  GemmBArgs a{};
  a.A = (const bf16_t*)a_in; a.W = (const bf16_t*)w; a.M = m; a.N = 3 * dim; a.K = k;
  a.bias = b;
  a.out = (bf16_t*)scratch;
  a.out_lo = a.out + L.ql;
  a.vt = a.out + L.vh;
  a.vt_lo = a.out + L.vl;
  a.dim = dim; a.heads = heads; a.s_pad = s_pad; a.vt_rows = batch * s_pad;
  return launch_gemm<EPI_QKV_X3>(a, (hipStream_t)stream);
}
