// Attention of the ViT extractor for gfx950 (head_dim 64): flash-style, S^T = K.Q^T so that the softmax statistics of a query
// live in one lane column and P is already in B-operand layout for O^T = V^T.P^T; bf16 operands on
// v_mfma_f32_16x16x32_bf16, fp32 softmax and accumulation.  q | k arrive as qk [batch*s_pad, 2*dim] (head-major inside), V
// TRANSPOSED per head as vt [batch, heads, 64, s_pad], both written by the qkv GEMM's epilogue (dvt_vit_gemm.hip).
//
// One body, attention_v2_body<VAR, X3>, behind an experiment mask; kernels the product launches from here:
//   attention_kernel_l2<559>   dvt_vit_attention_log2q: q pre-scaled by log2(e) / 8, the log2-domain loop -- what
//                              dvt_vit_forward runs (vit_attn_q_prescaled; dvt_tune_set(1, -531), the default)
//   attention_kernel_v2<15>    dvt_vit_attention: q as it is (dvt_tune_set(1, -530), and every direct caller)
//   attention_kernel_v2_x3     dvt_vit_attention_x3 / _x3_presplit: (hi, lo) bf16 operands, the fp32 extractor's bf16x3 mode
//   qk_split_kernel, v_split_transpose_kernel   dvt_vit_attention_x3: fp32 qkv rows -> the (hi, lo) operands
// The developer build (-DDVT_LAB) adds the round-2 kernel, the other masks and their dispatch (lab/dvt_vit_lab_attn.inc).
#include <type_traits>

#include "dvt_vit_dev.h"

namespace {

__device__ __forceinline__ float max3f(float a, float b, float c) {
  return __builtin_fmaxf(__builtin_fmaxf(a, b), c);  // v_max3_f32
}

// ======================================================================================
// Attention (head_dim 64): one workgroup = 128 queries of one (image, head); 8 waves x 16 queries
// ======================================================================================
constexpr int KV_TILE = 64;
// V^T tile in LDS: 64 rows (d) x 128 B, keys PERMUTED inside a row so that the 8 keys a lane feeds into one
// MFMA k-step -- {4g .. 4g+3} and {16+4g .. 16+4g+3} of the step's 32, the order in which the S^T accumulators
// hold P -- are 16 contiguous bytes (logical chunk 4 ks + g), and the chunk index XOR-ed with (row >> 1) & 7:
// ONE conflict-free ds_read_b128 per fragment.  (Before: four 8-byte reads per fragment pair that the compiler
// merged into ds_read2_b64 -- half the LDS rate, 32-bank mode, 2-way conflicts at the 144-B pitch.  PMC:
// SQ_LDS_BANK_CONFLICT 1.9e8 cycles per launch, the LDS pipe busier than the matrix pipe.)
constexpr int VT_LD = 128;

// ---- attention, round 3 ("v2"): the same tiling (128 queries per workgroup, 16 per wave, 64-key tiles, S^T = K.Q^T,
// O^T = V^T.P^T, register-staged K / V^T tiles) with the two serial chains of the v1 loop taken apart:
//   (1) S(t+1) is issued BEFORE the softmax of tile t.  In v1 a wave ran  S MFMAs -> softmax VALU -> PV MFMAs  strictly
//       in sequence, and the per-tile barrier keeps the 8 waves of a workgroup in lock step, so the matrix pipe idled
//       while everybody was in the softmax (SQ_VALU_MFMA_BUSY 22 %).  Now the 8 S MFMAs of the NEXT tile are
//       interleaved with the softmax of the CURRENT one (sched_group_barrier: one MFMA per ~7 VALU), their results are
//       needed an iteration later.  K therefore runs one tile further ahead: three K buffers, two V^T buffers (40 KB).
//   (2) deferred running max (the guide's T13).  A query's 64 keys of a tile live in 4 lanes; v1 reduced the tile max
//       across them with two dependent ds_bpermute round trips, recomputed alpha = exp(m_old - m_new) and rescaled l on
//       EVERY tile.  Now every lane only compares its own 16 logits with the running max: while no logit of the whole
//       wave exceeds it by more than THR = 8 (a wave vote, v_cmp + s_cbranch), nothing is reduced or rescaled and
//       P = exp(s - m_run) <= e^8 (bf16 keeps its relative precision there; accumulation is fp32).  Otherwise -- the
//       first tile, and rarely later -- the exact max is formed with v_permlane16/32_swap (no LDS) and o, l are rescaled.
//       tests/test_gpu_vit.py forces the late-rescale branch with a spiked key row (guide 5.4 rule 26).
constexpr int ATT2_KBUF = 3;

// VAR: experiment mask on top of the v2 structure (dvt_tune_set(1, -510 - mask); 0 = v2 as measured in r03):
//   1  S MFMAs issued k-step-major (the two MFMAs of one accumulator four MFMA slots apart instead of adjacent)
//   2  P.V: all eight V^T fragments read first, MFMAs accumulator-major per k-half (same-accumulator distance 4)
//   4  no per-tile max tree: P is formed against the running max and the tile is redone exactly only when a lane's
//      row sum leaves [0, e^8] (first tile: -1e30 running max -> inf -> exact path)
//   8  tile loop unrolled by two (S / S-next swap roles instead of being copied)
//   16 static priority for the second-dispatched half of the workgroup (waves 4-7)
//   64 two barriers per tile, waves 4-7 one phase behind waves 0-3 (softmax of one group over P.V of the other)
//   32 (round 6, needs 4) "log2 domain": q arrives PRE-SCALED by log2(e) / 8 (the qkv GEMM's epilogue does it on the fp32
//      accumulators, one rounding to bf16 as before), so S' = K.Q'^T is the logit in units of log2, and the S MFMA chain starts
//      from C = -m (the running max, one register quad) instead of 0: the accumulators hold t = s' - m and P = v_exp_f32(t)
//      with NO scale-and-subtract FMA (8 v_pk_fma_f32 of a tile's ~45 VALU issues; the kernel is VALU-issue bound: 16 quarter-rate
//      v_exp + ~30 others against 16 MFMAs per wave and tile).  Tile 0's exact max is formed in the prologue; when the running
//      max grows later (rare: the lane's 16-term row sum left [0, e^8]) this tile's t AND the already issued next tile's are
//      lowered by the growth.  Waves wholly behind the image's rows (s_pad < the block's 128 queries) stage and synchronise
//      but neither multiply nor exponentiate, and a last tile with <= 32 valid keys runs its softmax and P.V on half a tile.
//      Four K buffers and a tile loop unrolled by four (every buffer index a literal), staging unconditional with clamped tile
//      indices.  128 / 256: ablation builds (idle waves compute / whole tail tile).
//   512 (with 32) the scheduler's group pattern for the softmax block also places the next tile's K fragment READS: four up
//      front, then per MFMA slot 4 VALU, the MFMA, one read.  Left alone the reads sink behind the burst of 16 v_exp and every
//      MFMA waits out its own read (profiles/r06/r06s_*: 2856 -> 2799 us per 396-view launch).  The product launches 559 =
//      1 + 2 + 4 + 8 + 32 + 512.
// X3 (the fp32 extractor's opt-in "bf16x3" mode, include/dvt_vit.h): q, k, v arrive as (hi, lo) bf16 pairs of the fp32
// values (qk / vt = hi, qk_lo / vt_lo = lo), S = K_lo.Q_hi + K_hi.Q_lo + K_hi.Q_hi and O += V_lo.P_hi + V_hi.P_lo + V_hi.P_hi
// with P split in registers (3 x the MFMAs, fp32 accumulation, fp32 softmax as before) and `out` is fp32 [T, dim].
template <int VAR, bool X3>
__device__ __forceinline__ void attention_v2_body(const bf16_t* __restrict__ qk, const bf16_t* __restrict__ vt,
                                                  bf16_t* __restrict__ out, int heads, int s_pad, int n_valid,
                                                  const bf16_t* __restrict__ qk_lo, const bf16_t* __restrict__ vt_lo,
                                                  int split_out = 0) {
  constexpr int NV = (VAR & 64) ? 3 : 2;  // V^T buffers: the half-tile offset of the two wave groups needs a third
  constexpr bool L2D = (VAR & 32) != 0;
  constexpr bool SKIPW = L2D && !(VAR & 128), HALFT = L2D && !(VAR & 256);  // (128 / 256: ablation builds without the idle waves / the half tail tile)
  static_assert(!L2D || ((VAR & 4) && !X3 && !(VAR & 64)), "log2-domain build: on the no-max-tree structure, bf16 only");
  // K buffers: three suffice (K runs two tiles ahead); the log2-domain build takes FOUR and walks the tiles in an unrolled
  // loop of four whose counter is a multiple of 4, so that every buffer index ((kt + c) & 3, (kt + c) & 1) is a literal and the
  // LDS addresses are lane constants + immediates (with three buffers each tile spent ~8 VALU + SALU issues on slot offsets)
  constexpr int KBUF = L2D ? 4 : ATT2_KBUF;
  constexpr int KSET = KBUF * KV_TILE * 128, VSET = NV * 64 * VT_LD;  // one precision part: 24 (32) KB + 16 KB
  __shared__ __attribute__((aligned(16))) char smem[(X3 ? 2 : 1) * (KSET + VSET)];
  char* const Kb = smem;
  char* const Vb = smem + KSET;
  char* const Kbl = smem + KSET + VSET;  // X3: the lo parts
  char* const Vbl = Kbl + KSET;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, lc = lane & 15;
  const int nqb = (s_pad + ATT_Q - 1) / ATT_Q;  // the last block of an image may hang over its rows (s_pad % 16 == 0: whole waves)
  int id = blockIdx.x;
  {
    const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = id & 7, loc = id >> 3;
    id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  }
  const int qb = id % nqb, h = (id / nqb) % heads, b = id / (nqb * heads);
  const int dim = heads * 64, ldq = 2 * dim;
  const size_t row0 = (size_t)b * s_pad;

  bf16x8 qf[2], qfl[2];
  auto load_q = [&](const bf16_t* base, bf16x8 (&dst)[2]) {  // * head_dim^-0.5 = 2^-3: exact in bf16
    const bf16_t* qrow = base + (row0 + qb * ATT_Q + wave * 16 + lc) * ldq + h * 64;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      union { bf16x8 v; uint32_t u[4]; } raw;
      raw.v = *reinterpret_cast<const bf16x8*>(qrow + ks * 32 + g * 8);
      if constexpr (!L2D) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float lo = __uint_as_float(raw.u[j] << 16) * 0.125f;
          const float hi = __uint_as_float(raw.u[j] & 0xffff0000u) * 0.125f;
          raw.u[j] = pack2(lo, hi);
        }
      }
      dst[ks] = raw.v;
    }
  };
  load_q(qk, qf);
  if constexpr (X3) load_q(qk_lo, qfl);
  const bf16_t* kbase = qk + row0 * ldq + dim + h * 64;
  const bf16_t* vbase = vt + ((size_t)(b * heads + h) * 64) * s_pad;

  f32x4 o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m_run = L2D ? 0.f : -1e30f, l_run = 0.f;  // (L2D: in units of log2; tile 0's exact max is formed in the prologue)
  f32x4 cinit = (f32x4){0.f, 0.f, 0.f, 0.f};      // L2D: -m_run in every element, the C operand an S chain starts from
  const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
  // L2D: a wave whose 16 queries lie wholly behind the image's rows (the last block of an image where s_pad % 128 != 0)
  // only stages and synchronises (wave-uniform)
  const bool active = !SKIPW || qb * ATT_Q + __builtin_amdgcn_readfirstlane(wave) * 16 < s_pad;
  const float LOG2E = 1.4426950408889634f;
  const float THR = 8.0f;

  const int ntiles = (n_valid + KV_TILE - 1) / KV_TILE;
  const int sr0 = tid >> 3, sc = tid & 7;
  const bf16_t* kp0 = kbase + (size_t)sr0 * ldq + sc * 8;
  const bf16_t* vp0 = vbase + (size_t)sr0 * s_pad + sc * 8;
  const int kdo = sr0 * 128 + ((sc ^ (sr0 & 7)) << 4);
  const int vks = sc >> 2, vc = sc & 3, vsw = (sr0 >> 1) & 7;
  const int vdo0 = sr0 * VT_LD + (((vks * 4 + 2 * (vc & 1)) ^ vsw) << 4) + (vc >> 1) * 8;
  const int vdo1 = sr0 * VT_LD + (((vks * 4 + 2 * (vc & 1) + 1) ^ vsw) << 4) + (vc >> 1) * 8;
  uint4 kr0, vr0, kr0l, vr0l;
  const ptrdiff_t klo = X3 ? (qk_lo - qk) : 0, vlo = X3 ? (vt_lo - vt) : 0;  // element offsets hi -> lo arrays
  // L2D: staging loads as (wave-uniform base of the tile) + (32-bit lane offset): the base advances on the scalar unit, the
  // lane part is a loop constant (global_load saddr form; the 64-bit per-lane pointers above cost a v_lshl_add_u64 per load)
  const unsigned klane = (unsigned)(sr0 * ldq + sc * 8) * 2u;
  const unsigned vlane = (unsigned)(sr0 * s_pad + sc * 8) * 2u, vlane0 = (unsigned)(sr0 * s_pad) * 2u;
#define A2_LOADK(kt)                                                                                 \
  do {                                                                                               \
    if constexpr (L2D) {                                                                             \
      kr0 = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(kbase + (size_t)(kt) * KV_TILE * ldq) + klane); \
    } else {                                                                                         \
      kr0 = *reinterpret_cast<const uint4*>(kp0 + (size_t)(kt) * KV_TILE * ldq);                     \
    }                                                                                                \
    if constexpr (X3) kr0l = *reinterpret_cast<const uint4*>(kp0 + klo + (size_t)(kt) * KV_TILE * ldq); \
  } while (0)
// (a lane's 8 keys lie wholly inside or wholly behind the image's s_pad keys (s_pad % 8 == 0).  Behind them -- the last tile
// where s_pad % 64 != 0 -- the lane re-reads a chunk of real keys instead: those keys' P is 0, but what lies behind a V^T row
// is the next row / head / image or unwritten workspace, and 0 x NaN would poison the row's output.  "Re-reads": the row's
// first chunk, which always exists)
// (L2D: the lane re-reads chunk 0 of the SAME tile -- kt * 64 < n_valid <= s_pad, both multiples of 8 -- so that the address
// stays tile base + a non-negative lane offset)
#define A2_LOADV(kt)                                                                   \
  do {                                                                                 \
    if constexpr (L2D) {                                                               \
      const unsigned vo_ = (kt) * KV_TILE + sc * 8 >= s_pad ? vlane0 : vlane;          \
      vr0 = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(vbase + (kt) * KV_TILE) + vo_); \
    } else {                                                                           \
      const int vk_ = (kt) * KV_TILE + sc * 8 >= s_pad ? -sc * 8 : (kt) * KV_TILE;     \
      vr0 = *reinterpret_cast<const uint4*>(vp0 + vk_);                                \
      if constexpr (X3) vr0l = *reinterpret_cast<const uint4*>(vp0 + vlo + vk_);       \
    }                                                                                  \
  } while (0)
#define A2_STOREK(kt)                                                                                   \
  do {                                                                                                  \
    *reinterpret_cast<uint4*>(Kb + ((kt) % KBUF) * (KV_TILE * 128) + kdo) = kr0;                   \
    if constexpr (X3) *reinterpret_cast<uint4*>(Kbl + ((kt) % KBUF) * (KV_TILE * 128) + kdo) = kr0l; \
  } while (0)
#define A2_STOREV(kt)                                                                     \
  do {                                                                                    \
    char* vb_ = Vb + ((kt) % NV) * (64 * VT_LD);                                          \
    *reinterpret_cast<uint2*>(vb_ + vdo0) = make_uint2(vr0.x, vr0.y);                     \
    *reinterpret_cast<uint2*>(vb_ + vdo1) = make_uint2(vr0.z, vr0.w);                     \
    if constexpr (X3) {                                                                   \
      char* vl_ = Vbl + ((kt) % NV) * (64 * VT_LD);                                       \
      *reinterpret_cast<uint2*>(vl_ + vdo0) = make_uint2(vr0l.x, vr0l.y);                 \
      *reinterpret_cast<uint2*>(vl_ + vdo1) = make_uint2(vr0l.z, vr0l.w);                 \
    }                                                                                     \
  } while (0)
  // S^T of tile kt: acc s[mt][r] <-> key = 16*mt + 4*g + r, q = lc
#define A2_S(dst, kt)                                                                                              \
  do {                                                                                                             \
    const char* Ks_ = Kb + ((kt) % KBUF) * (KV_TILE * 128);                                                   \
    if constexpr (X3) {                                                                                            \
      const char* Kl_ = Kbl + ((kt) % KBUF) * (KV_TILE * 128);                                                \
      _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                                           \
        bf16x8 kh_[4], kl_[4];                                                                                     \
        _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) {                                                         \
          const int krow = mt * 16 + lc, ko_ = krow * 128 + (((ks * 4 + g) ^ (krow & 7)) << 4);                     \
          kh_[mt] = *reinterpret_cast<const bf16x8*>(Ks_ + ko_);                                                   \
          kl_[mt] = *reinterpret_cast<const bf16x8*>(Kl_ + ko_);                                                   \
          if (ks == 0) dst[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};                                                      \
        }                                                                                                          \
        _Pragma("unroll") for (int mt = 0; mt < 4; ++mt)                                                           \
          dst[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl_[mt], qf[ks], dst[mt], 0, 0, 0);                    \
        _Pragma("unroll") for (int mt = 0; mt < 4; ++mt)                                                           \
          dst[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh_[mt], qfl[ks], dst[mt], 0, 0, 0);                   \
        _Pragma("unroll") for (int mt = 0; mt < 4; ++mt)                                                           \
          dst[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh_[mt], qf[ks], dst[mt], 0, 0, 0);                    \
      }                                                                                                            \
    } else if constexpr (VAR & 1) {                                                                                       \
      _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                                           \
        _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) {                                                         \
          const int krow = mt * 16 + lc;                                                                           \
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks_ + krow * 128 + (((ks * 4 + g) ^ (krow & 7)) << 4)); \
          if (ks == 0) dst[mt] = L2D ? cinit : zero4;                                                              \
          dst[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], dst[mt], 0, 0, 0);                         \
        }                                                                                                          \
      }                                                                                                            \
    } else {                                                                                                       \
    _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) {                                                             \
      dst[mt] = L2D ? cinit : zero4;                                                                               \
      _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                                           \
        const int krow = mt * 16 + lc;                                                                             \
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks_ + krow * 128 + (((ks * 4 + g) ^ (krow & 7)) << 4)); \
        dst[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], dst[mt], 0, 0, 0);                           \
      }                                                                                                            \
    }                                                                                                              \
    }                                                                                                              \
  } while (0)

  // prologue: K0, V0, K1 staged; S(0); K2 / V1 in flight in registers
  A2_LOADK(0);
  A2_LOADV(0);
  A2_STOREK(0);
  A2_STOREV(0);
  if constexpr (L2D) {  // (tile indices clamped to the last tile, see the tile body)
    const int last = ntiles - 1;
    A2_LOADK(1 < last ? 1 : last);
    A2_STOREK(1);
    A2_LOADK(2 < last ? 2 : last);
    A2_LOADV(1 < last ? 1 : last);
  } else {
    if (ntiles > 1) {
      A2_LOADK(1);
      A2_STOREK(1);
    }
    if (ntiles > 2) A2_LOADK(2);
    if (ntiles > 1) A2_LOADV(1);
  }
  __syncthreads();
  f32x4 sA[4], sB[4];
  // the exact maximum of a query's logits over its 4 lanes (lc + 16 g): swap rows 0<->1 / 2<->3, then the wave halves (no LDS)
  auto lane_quad_max = [&](float v) {
    const unsigned u = __float_as_uint(v);
    const auto r16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v = fmaxf(__uint_as_float(r16[0]), __uint_as_float(r16[1]));
    const unsigned u2 = __float_as_uint(v);
    const auto r32 = __builtin_amdgcn_permlane32_swap(u2, u2, false, false);
    return fmaxf(__uint_as_float(r32[0]), __uint_as_float(r32[1]));
  };
  auto max16 = [&](const f32x4 (&s)[4]) {
    float tmax = __builtin_fmaxf(__builtin_fmaxf(s[0][0], s[0][1]), s[0][2]);
    tmax = max3f(tmax, s[0][3], s[1][0]);
    tmax = max3f(tmax, s[1][1], s[1][2]);
    tmax = max3f(tmax, s[1][3], s[2][0]);
    tmax = max3f(tmax, s[2][1], s[2][2]);
    tmax = max3f(tmax, s[2][3], s[3][0]);
    tmax = max3f(tmax, s[3][1], s[3][2]);
    return fmaxf(tmax, s[3][3]);
  };
  if (active) A2_S(sA, 0);
  if constexpr (L2D) {
    if (active) {
      // tile 0: the running max starts at the tile's exact max (every later tile only checks that nothing grew past e^8)
      if (n_valid < KV_TILE) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (mt * 16 + 4 * g + r >= n_valid) sA[mt][r] = -1e30f;
      }
      m_run = lane_quad_max(max16(sA));
      cinit = (f32x4){-m_run, -m_run, -m_run, -m_run};
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) sA[mt] += cinit;
    }
  }
  if constexpr (VAR & 16) {
    if (wave >= 4) __builtin_amdgcn_s_setprio(1);
  }
  if constexpr (VAR & 64) {
    // ping-pong: waves 4-7 (the second wave of every SIMD) run one phase behind waves 0-3, so that one group's
    // softmax (VALU) phase meets the other group's P.V (MFMA + LDS) phase on every SIMD
    if (wave >= 4) __syncthreads();
  }
  union PF { bf16x8 v; uint32_t u[4]; };
  // one tile.  LAST: the final tile (padding keys masked, no next tile to start).  From the vote onwards the body of
  // the common case is ONE basic block, so that the scheduler hints can interleave the next tile's S MFMAs with it.
  // (Tried and dropped, profiles/r03: also deferring P.V by one tile so that the block carries 16 independent MFMAs --
  // +1 % with hints, -7 % with a hand-placed MFMA / exp interleave whose LDS reads ran only two slots ahead.)
  auto tile = [&](int kt, auto last_tag, f32x4 (&s)[4], f32x4 (&sn)[4]) {
    constexpr bool LAST = decltype(last_tag)::value;
    if constexpr (L2D) {
      // unconditional staging (no branches, no phis around the in-flight registers): behind the last tile the LAST tile is
      // loaded again and lands in buffers nobody reads any more (K: four buffers, the readers are at (kt + 1) & 3 at most; V^T:
      // the buffer this tile does not read)
      const int last = ntiles - 1;
      A2_STOREK(kt + 2);
      A2_STOREV(kt + 1);
      if constexpr (!LAST) {
        const int k3 = kt + 3 < last ? kt + 3 : last, v2 = kt + 2 < last ? kt + 2 : last;
        A2_LOADK(k3);
        A2_LOADV(v2);
      }
    } else {
    if (kt + 2 < ntiles) A2_STOREK(kt + 2);  // loaded an iteration ago; that buffer was last read two barriers back
    if (kt + 1 < ntiles) A2_STOREV(kt + 1);
    if (kt + 3 < ntiles) A2_LOADK(kt + 3);
    if (kt + 2 < ntiles) A2_LOADV(kt + 2);
    }
    if constexpr (LAST) {
      const int kbase_idx = kt * KV_TILE;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (kbase_idx + mt * 16 + 4 * g + r >= n_valid) s[mt][r] = -1e30f;
    }
    // exact running max over the query's 4 lanes (lc + 16 g) + rescale of o, l (everything still at the old max is scaled
    // exactly once: P.V of the previous tile is complete)
    auto exact_max = [&]() {
      if constexpr (L2D) {
        // s holds t = s' - m_run: the max grows by d = max(t) where that is positive; everything that was formed against
        // the old max is lowered by d -- o and l (scaled by 2^-d; P.V of the previous tile is complete), this tile's t, and
        // the NEXT tile's, whose chain already started from the old -m_run
        const float d = fmaxf(lane_quad_max(max16(s)), 0.f);
        const float alpha = __builtin_amdgcn_exp2f(-d);
        l_run *= alpha;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] *= alpha;
        m_run += d;
        cinit = (f32x4){-m_run, -m_run, -m_run, -m_run};
        const f32x4 d4 = {d, d, d, d};
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          s[mt] -= d4;
          if constexpr (!LAST) sn[mt] -= d4;
        }
        return;
      }
      float tmax = __builtin_fmaxf(__builtin_fmaxf(s[0][0], s[0][1]), s[0][2]);
      tmax = max3f(tmax, s[0][3], s[1][0]);
      tmax = max3f(tmax, s[1][1], s[1][2]);
      tmax = max3f(tmax, s[1][3], s[2][0]);
      tmax = max3f(tmax, s[2][1], s[2][2]);
      tmax = max3f(tmax, s[2][3], s[3][0]);
      tmax = max3f(tmax, s[3][1], s[3][2]);
      tmax = fmaxf(tmax, s[3][3]);
      const unsigned u = __float_as_uint(tmax);
      const auto r16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
      tmax = fmaxf(__uint_as_float(r16[0]), __uint_as_float(r16[1]));
      const unsigned u2 = __float_as_uint(tmax);
      const auto r32 = __builtin_amdgcn_permlane32_swap(u2, u2, false, false);
      tmax = fmaxf(__uint_as_float(r32[0]), __uint_as_float(r32[1]));
      const float m_new = fmaxf(m_run, tmax);
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E);
      l_run *= alpha;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o[i][0] *= alpha;
        o[i][1] *= alpha;
        o[i][2] *= alpha;
        o[i][3] *= alpha;
      }
      m_run = m_new;
    };
    if constexpr (!(VAR & 4)) {
    float tmax = __builtin_fmaxf(__builtin_fmaxf(s[0][0], s[0][1]), s[0][2]);
      tmax = max3f(tmax, s[0][3], s[1][0]);
      tmax = max3f(tmax, s[1][1], s[1][2]);
      tmax = max3f(tmax, s[1][3], s[2][0]);
      tmax = max3f(tmax, s[2][1], s[2][2]);
      tmax = max3f(tmax, s[2][3], s[3][0]);
      tmax = max3f(tmax, s[3][1], s[3][2]);
      tmax = fmaxf(tmax, s[3][3]);
      if (!__all(tmax <= m_run + THR)) {  // wave-uniform, rare after the first tile
        // exact max over the query's 4 lanes (lc + 16 g): swap rows 0<->1 / 2<->3, then the wave halves
        const unsigned u = __float_as_uint(tmax);
        const auto r16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
        tmax = fmaxf(__uint_as_float(r16[0]), __uint_as_float(r16[1]));
        const unsigned u2 = __float_as_uint(tmax);
        const auto r32 = __builtin_amdgcn_permlane32_swap(u2, u2, false, false);
        tmax = fmaxf(__uint_as_float(r32[0]), __uint_as_float(r32[1]));
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E);
        l_run *= alpha;  // everything still at the old max is scaled exactly once: o and l (P.V of the previous tile is complete)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          o[i][0] *= alpha;
          o[i][1] *= alpha;
          o[i][2] *= alpha;
          o[i][3] *= alpha;
        }
        m_run = m_new;
      }
    }
    if constexpr (HALFT && LAST) {
      if (n_valid - kt * KV_TILE <= 32) {
        // (wave-uniform) keys 32..63 of the last tile are all padding (ViT-B/14 at 518 px: 1370 = 21 x 64 + 26): softmax, pack
        // and P.V on the tile's first k-half only -- 8 v_exp, one P fragment, 4 V^T fragments, 4 MFMAs
        float hp[2][4];
        f32x2 hs2;
        auto half_softmax = [&]() {
          hs2 = (f32x2){0.f, 0.f};
#pragma unroll
          for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
              f32x2 e;
              e.x = __builtin_amdgcn_exp2f(s[mt][2 * h2]);
              e.y = __builtin_amdgcn_exp2f(s[mt][2 * h2 + 1]);
              hs2 += e;
              hp[mt][2 * h2] = e.x;
              hp[mt][2 * h2 + 1] = e.y;
            }
        };
        half_softmax();
        float hsum = hs2.x + hs2.y;
        if (!__all(hsum <= 2980.0f)) {
          exact_max();
          half_softmax();
          hsum = hs2.x + hs2.y;
        }
        l_run += hsum;
        union { bf16x8 v; uint32_t u[4]; } hf;
        hf.u[0] = pack2(hp[0][0], hp[0][1]); hf.u[1] = pack2(hp[0][2], hp[0][3]);
        hf.u[2] = pack2(hp[1][0], hp[1][1]); hf.u[3] = pack2(hp[1][2], hp[1][3]);
        const char* Vh = Vb + (kt % NV) * (64 * VT_LD);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          const int vr = mt * 16 + lc, vs_ = (vr >> 1) & 7;
          const bf16x8 vf = *reinterpret_cast<const bf16x8*>(Vh + vr * VT_LD + ((g ^ vs_) << 4));
          o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, hf.v, o[mt], 0, 0, 0);
        }
        __syncthreads();
        return;
      }
    }
    if constexpr (L2D && !LAST && (VAR & 16384)) {
      // (experiment, 16384) the softmax SPLIT over the tile's two blocks, so that both carry matrix work AND exps: block 1 = the
      // next tile's 8 S MFMAs beside the exps of keys 0..31 (P fragment 0); block 2 = the first four P.V MFMAs (fragment 0)
      // beside the exps of keys 32..63 (fragment 1), then the other four.  Each half has its own lane-sum vote.  A growth of
      // the max found by the SECOND vote rescales o and l -- which then already hold the first half's contribution, formed
      // against the same old max and finite (its vote passed): scaled by the same 2^-d it is what the new max asks for.
      union PH { bf16x8 v; uint32_t u[4]; };
      float hp[4][4];
      auto soft_half = [&](int h) {
        f32x2 a2, b2;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int mt = 2 * h + q;
          f32x2 e0, e1;
          e0.x = __builtin_amdgcn_exp2f(s[mt][0]);
          e0.y = __builtin_amdgcn_exp2f(s[mt][1]);
          e1.x = __builtin_amdgcn_exp2f(s[mt][2]);
          e1.y = __builtin_amdgcn_exp2f(s[mt][3]);
          if (q == 0) {
            a2 = e0;
            b2 = e1;
          } else {
            a2 += e0;
            b2 += e1;
          }
          hp[mt][0] = e0.x; hp[mt][1] = e0.y; hp[mt][2] = e1.x; hp[mt][3] = e1.y;
        }
        a2 += b2;
        return a2.x + a2.y;
      };
      auto pack_half = [&](int h, PH& f) {
        f.u[0] = pack2(hp[2 * h][0], hp[2 * h][1]); f.u[1] = pack2(hp[2 * h][2], hp[2 * h][3]);
        f.u[2] = pack2(hp[2 * h + 1][0], hp[2 * h + 1][1]); f.u[3] = pack2(hp[2 * h + 1][2], hp[2 * h + 1][3]);
      };
      PH f0, f1;
      __builtin_amdgcn_sched_barrier(0);
      A2_S(sn, kt + 1);
      float ps = soft_half(0);
      pack_half(0, f0);
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (i < 4) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (!__all(ps <= 2980.0f)) {
        exact_max();
        ps = soft_half(0);
        pack_half(0, f0);
      }
      l_run += ps;
      const char* Vs2 = Vb + (kt % NV) * (64 * VT_LD);
      bf16x8 vf[8];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int vr = mt * 16 + lc, vs_ = (vr >> 1) & 7;
        const char* vrow = Vs2 + vr * VT_LD;
        vf[mt] = *reinterpret_cast<const bf16x8*>(vrow + ((g ^ vs_) << 4));
        vf[4 + mt] = *reinterpret_cast<const bf16x8*>(vrow + (((4 + g) ^ vs_) << 4));
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[mt], f0.v, o[mt], 0, 0, 0);
      float ps1 = soft_half(1);
      pack_half(1, f1);
      __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (!__all(ps1 <= 2980.0f)) {
        exact_max();  // (o and l: the first half's share included, see above)
        ps1 = soft_half(1);
        pack_half(1, f1);
      }
      l_run += ps1;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[4 + mt], f1.v, o[mt], 0, 0, 0);
      __syncthreads();
      return;
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (VAR & 4096) __builtin_amdgcn_s_setprio(1);  // (experiment) ... or the S / softmax block does
    if constexpr (!LAST) A2_S(sn, kt + 1);  // K(kt+1) became visible at the previous barrier (or in the prologue)
    const f32x2 l2e2 = {LOG2E, LOG2E};
    float pv[4][4];
    f32x2 ps2;
    auto softmax = [&]() {
      const float mb = m_run * LOG2E;
      const f32x2 nmb2 = {-mb, -mb};
      f32x2 psb;  // L2D: two chains of four packed adds (a single chain of eight needs a wait state between any two), started
                  // from the first pairs instead of 0 + e
      if constexpr (!L2D) ps2 = (f32x2){0.f, 0.f};
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          const f32x2 sv = {s[mt][2 * h2], s[mt][2 * h2 + 1]};
          const f32x2 t = L2D ? sv : __builtin_elementwise_fma(sv, l2e2, nmb2);
          f32x2 e;
          e.x = __builtin_amdgcn_exp2f(t.x);
          e.y = __builtin_amdgcn_exp2f(t.y);
          if constexpr (L2D) {
            if (mt == 0) (h2 == 0 ? ps2 : psb) = e;
            else (h2 == 0 ? ps2 : psb) += e;
          } else {
            ps2 += e;
          }
          pv[mt][2 * h2] = e.x;
          pv[mt][2 * h2 + 1] = e.y;
        }
      if constexpr (L2D) ps2 += psb;
    };
    softmax();
    float psum = ps2.x + ps2.y;
    PF pf0, pf1, pl0, pl1;
    auto pack = [&]() {
      pf0.u[0] = pack2(pv[0][0], pv[0][1]); pf0.u[1] = pack2(pv[0][2], pv[0][3]);
      pf0.u[2] = pack2(pv[1][0], pv[1][1]); pf0.u[3] = pack2(pv[1][2], pv[1][3]);
      pf1.u[0] = pack2(pv[2][0], pv[2][1]); pf1.u[1] = pack2(pv[2][2], pv[2][3]);
      pf1.u[2] = pack2(pv[3][0], pv[3][1]); pf1.u[3] = pack2(pv[3][2], pv[3][3]);
      if constexpr (X3) {  // P = hi + lo: lo = bf16(p - float(hi)), the subtraction is exact
        auto lo2 = [](uint32_t hb, float a, float b) {
          return pack2(a - __uint_as_float(hb << 16), b - __uint_as_float(hb & 0xffff0000u));
        };
        pl0.u[0] = lo2(pf0.u[0], pv[0][0], pv[0][1]); pl0.u[1] = lo2(pf0.u[1], pv[0][2], pv[0][3]);
        pl0.u[2] = lo2(pf0.u[2], pv[1][0], pv[1][1]); pl0.u[3] = lo2(pf0.u[3], pv[1][2], pv[1][3]);
        pl1.u[0] = lo2(pf1.u[0], pv[2][0], pv[2][1]); pl1.u[1] = lo2(pf1.u[1], pv[2][2], pv[2][3]);
        pl1.u[2] = lo2(pf1.u[2], pv[3][0], pv[3][1]); pl1.u[3] = lo2(pf1.u[3], pv[3][2], pv[3][3]);
      }
    };
    if constexpr (!(VAR & 1024)) pack();
    if constexpr (!LAST && (VAR & 32768)) {
      // (experiment) LLVM's own interleaving strategies for this block instead of the group pattern: 2 = MFMAExpInterleave,
      // written for exp-heavy attention loops (VAR & 65536: 3 = its simple form)
      __builtin_amdgcn_iglp_opt((VAR & 65536) ? 3 : 2);
    } else if constexpr (!LAST && (VAR & 512)) {
      // (experiment) the K fragment reads placed too: four up front, then per MFMA slot 4 VALU, the MFMA, the read that
      // re-fills its fragment registers -- left alone the reads sink behind the exps and every MFMA waits for its own read
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (i < 4) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
    } else if constexpr (!LAST) {
      // scheduler shape for the block above: one S MFMA of the next tile per ~6 VALU of this tile's softmax
#pragma unroll
      for (int i = 0; i < (X3 ? 24 : 8); ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, (X3 || L2D) ? 4 : (VAR & 4) ? 5 : 6, 0);  // VALU
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (VAR & 4096) __builtin_amdgcn_s_setprio(0);
    if constexpr (VAR & 4) {
      // every P of this lane is within [0, e^8] iff its 16-term sum is (terms are >= 0; inf / NaN fail the compare)
      if (!__all(psum <= 2980.0f)) {
        exact_max();
        softmax();
        psum = ps2.x + ps2.y;
        if constexpr (!(VAR & 1024)) pack();
      }
    }
    l_run += psum;
    // ---- O^T[d][q] += V^T . P^T
    if constexpr (VAR & 64) __syncthreads();  // phase boundary: the other wave group starts its softmax phase here
    const char* Vs = Vb + (kt % NV) * (64 * VT_LD);
    if constexpr (X3) {
      const char* Vl = Vbl + (kt % NV) * (64 * VT_LD);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int vr = mt * 16 + lc, vs_ = (vr >> 1) & 7;
        const int o0_ = vr * VT_LD + ((g ^ vs_) << 4), o1_ = vr * VT_LD + (((4 + g) ^ vs_) << 4);
        const bf16x8 vh0 = *reinterpret_cast<const bf16x8*>(Vs + o0_), vh1 = *reinterpret_cast<const bf16x8*>(Vs + o1_);
        const bf16x8 vl0 = *reinterpret_cast<const bf16x8*>(Vl + o0_), vl1 = *reinterpret_cast<const bf16x8*>(Vl + o1_);
        o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vl0, pf0.v, o[mt], 0, 0, 0);
        o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vl1, pf1.v, o[mt], 0, 0, 0);
        o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh0, pl0.v, o[mt], 0, 0, 0);
        o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh1, pl1.v, o[mt], 0, 0, 0);
        o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh0, pf0.v, o[mt], 0, 0, 0);
        o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh1, pf1.v, o[mt], 0, 0, 0);
      }
    } else if constexpr (VAR & 2) {
      if constexpr (VAR & 2048) __builtin_amdgcn_s_setprio(1);  // (experiment) the P.V block wins the issue arbitration
      bf16x8 vf[8];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int vr = mt * 16 + lc, vs_ = (vr >> 1) & 7;
        const char* vrow = Vs + vr * VT_LD;
        vf[mt] = *reinterpret_cast<const bf16x8*>(vrow + ((g ^ vs_) << 4));
        vf[4 + mt] = *reinterpret_cast<const bf16x8*>(vrow + (((4 + g) ^ vs_) << 4));
      }
      if constexpr (VAR & 1024) pack();  // (experiment) P is packed BEHIND the V^T fragment reads: the eight v_cvt_pk cover their latency
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[mt], pf0.v, o[mt], 0, 0, 0);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[4 + mt], pf1.v, o[mt], 0, 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);  // the eight LDS reads
      if constexpr (VAR & 1024) __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);  // the eight v_cvt_pk
      __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);  // then the MFMAs in source order
      if constexpr (VAR & 2048) __builtin_amdgcn_s_setprio(0);
    } else {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int vr = mt * 16 + lc, vs_ = (vr >> 1) & 7;
        const char* vrow = Vs + vr * VT_LD;
        const bf16x8 vf0 = *reinterpret_cast<const bf16x8*>(vrow + ((g ^ vs_) << 4));
        const bf16x8 vf1 = *reinterpret_cast<const bf16x8*>(vrow + (((4 + g) ^ vs_) << 4));
        o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf0, pf0.v, o[mt], 0, 0, 0);
        o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf1, pf1.v, o[mt], 0, 0, 0);
      }
    }
    if constexpr (VAR & 8192) {  // TIMING ONLY (developer library): no tile barrier -- what the lock step of a workgroup's 8 waves costs
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    } else {
      __syncthreads();
    }
  };
  if constexpr (SKIPW) {
    if (!active) {
      // an idle wave's loop: its share of the staging and the tile barriers (s_barrier counts arrivals, whatever the PC)
      const int last = ntiles - 1;
      for (int kt = 0; kt < ntiles; ++kt) {
        A2_STOREK(kt + 2);
        A2_STOREV(kt + 1);
        A2_LOADK(kt + 3 < last ? kt + 3 : last);
        A2_LOADV(kt + 2 < last ? kt + 2 : last);
        __syncthreads();
      }
      return;
    }
  }
  if constexpr (L2D) {
    int kt = 0;
    for (; kt + 4 <= ntiles - 1; kt += 4) {
      tile(kt, std::false_type{}, sA, sB);
      tile(kt + 1, std::false_type{}, sB, sA);
      tile(kt + 2, std::false_type{}, sA, sB);
      tile(kt + 3, std::false_type{}, sB, sA);
    }
    for (; kt < ntiles - 1; ++kt) {  // 0..3 whole tiles before the last one (buffer indices at run time)
      tile(kt, std::false_type{}, sA, sB);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) sA[mt] = sB[mt];
    }
    tile(ntiles - 1, std::true_type{}, sA, sB);
  } else if constexpr (VAR & 8) {
    int kt = 0;
    for (; kt + 2 <= ntiles - 1; kt += 2) {
      tile(kt, std::false_type{}, sA, sB);
      tile(kt + 1, std::false_type{}, sB, sA);
    }
    if (kt < ntiles - 1) {
      tile(kt, std::false_type{}, sA, sB);
      tile(ntiles - 1, std::true_type{}, sB, sA);
    } else {
      tile(ntiles - 1, std::true_type{}, sA, sB);
    }
  } else {
    for (int kt = 0; kt < ntiles - 1; ++kt) {
      tile(kt, std::false_type{}, sA, sB);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) sA[mt] = sB[mt];
    }
    tile(ntiles - 1, std::true_type{}, sA, sB);
  }
  if constexpr (VAR & 16) __builtin_amdgcn_s_setprio(0);
  if constexpr (VAR & 64) {
    if (wave < 4) __syncthreads();
  }
#undef A2_LOADK
#undef A2_LOADV
#undef A2_STOREK
#undef A2_STOREV
#undef A2_S
  if (qb * ATT_Q + wave * 16 >= s_pad) return;  // a wave past the image's rows (its 16 "queries" were the next image's): nothing to store
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  const float inv = 1.0f / l_run;
  if constexpr (X3) {
    if (split_out) {  // the proj GEMM's A row [hi | hi | lo] (3 dim wide) instead of fp32: no split pass in between
      bf16_t* r3 = out + (row0 + qb * ATT_Q + wave * 16 + lc) * (3 * dim) + h * 64;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const float a0 = o[mt][0] * inv, a1 = o[mt][1] * inv, a2 = o[mt][2] * inv, a3 = o[mt][3] * inv;
        uint2 hh, ll;
        hh.x = pack2(a0, a1);
        hh.y = pack2(a2, a3);
        ll.x = pack2(a0 - __uint_as_float(hh.x << 16), a1 - __uint_as_float(hh.x & 0xffff0000u));
        ll.y = pack2(a2 - __uint_as_float(hh.y << 16), a3 - __uint_as_float(hh.y & 0xffff0000u));
        bf16_t* c = r3 + mt * 16 + 4 * g;
        *reinterpret_cast<uint2*>(c) = hh;
        *reinterpret_cast<uint2*>(c + dim) = hh;
        *reinterpret_cast<uint2*>(c + 2 * dim) = ll;
      }
      return;
    }
    float* orow = reinterpret_cast<float*>(out) + (row0 + qb * ATT_Q + wave * 16 + lc) * dim + h * 64;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
      *reinterpret_cast<float4*>(orow + mt * 16 + 4 * g) =
          make_float4(o[mt][0] * inv, o[mt][1] * inv, o[mt][2] * inv, o[mt][3] * inv);
    return;
  }
  bf16_t* orow = out + (row0 + qb * ATT_Q + wave * 16 + lc) * dim + h * 64;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    uint2 pk;
    pk.x = pack2(o[mt][0] * inv, o[mt][1] * inv);
    pk.y = pack2(o[mt][2] * inv, o[mt][3] * inv);
    *reinterpret_cast<uint2*>(orow + mt * 16 + 4 * g) = pk;
  }
}

template <int VAR>
__global__ __launch_bounds__(512) void attention_kernel_v2(const bf16_t* __restrict__ qk, const bf16_t* __restrict__ vt,
                                                           bf16_t* __restrict__ out, int heads, int s_pad, int n_valid) {
  attention_v2_body<VAR, false>(qk, vt, out, heads, s_pad, n_valid, nullptr, nullptr);
}
// the log2-domain builds (VAR bit 32).  Left alone hipcc takes 134-136 registers for them (the -m quad, twice in the loop
// unrolled by two) = ONE workgroup per CU; told to fit four waves per SIMD it parks three dwords (the output row pointer, across
// the loop) and a few more in the last-tile code in scratch and keeps the tile loop free of scratch traffic (ISA checked).
template <int VAR>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void attention_kernel_l2(
    const bf16_t* __restrict__ qk, const bf16_t* __restrict__ vt, bf16_t* __restrict__ out, int heads, int s_pad, int n_valid) {
  static_assert(VAR & 32, "log2-domain builds only");
  attention_v2_body<VAR, false>(qk, vt, out, heads, s_pad, n_valid, nullptr, nullptr);
}
// the split-operand build: 156 registers, one 80-KB workgroup per CU (capped at 128 registers -- 24 dwords of scratch,
// two workgroups per CU -- it measured 1.71-1.76 ms per 64 views against 1.30-1.53: dropped)
__global__ __launch_bounds__(512) void attention_kernel_v2_x3(const bf16_t* __restrict__ qk, const bf16_t* __restrict__ vt,
                                                              bf16_t* __restrict__ out, int heads, int s_pad, int n_valid,
                                                              const bf16_t* __restrict__ qk_lo,
                                                              const bf16_t* __restrict__ vt_lo, int split_out) {
  attention_v2_body<12, true>(qk, vt, out, heads, s_pad, n_valid, qk_lo, vt_lo, split_out);
}

// ---- bf16x3 attention for the fp32 extractor's `--fp32_matmul high` mode ---------------------------------------
__device__ __forceinline__ void split_pair(float a, float b, uint32_t& hi, uint32_t& lo) {
  hi = pack2(a, b);
  lo = pack2(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
}
// q | k columns of the fp32 qkv rows -> (hi, lo) bf16 arrays [T, 2 dim]
__global__ __launch_bounds__(256) void qk_split_kernel(const float* __restrict__ qkv, bf16_t* __restrict__ hi,
                                                       bf16_t* __restrict__ lo, long long nq, int dq2, int ld3) {
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long long)gridDim.x * 256) {
    const long long t = q / dq2;
    const int c = (int)(q - t * dq2) * 4;
    const float4 v = *reinterpret_cast<const float4*>(qkv + t * ld3 + c);
    uint2 h, l;
    split_pair(v.x, v.y, h.x, l.x);
    split_pair(v.z, v.w, h.y, l.y);
    *reinterpret_cast<uint2*>(hi + t * (dq2 * 4) + c) = h;
    *reinterpret_cast<uint2*>(lo + t * (dq2 * 4) + c) = l;
  }
}
// v columns -> transposed (hi, lo) arrays vt[b][h][d][s]; one workgroup = 64 tokens of one (image, head)
__global__ __launch_bounds__(256) void v_split_transpose_kernel(const float* __restrict__ qkv, bf16_t* __restrict__ vth,
                                                                bf16_t* __restrict__ vtl, int heads, int s_pad) {
  __shared__ float tile[64 * 65];
  const int t0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int dim = heads * 64, ld3 = 3 * dim;
  const float* src = qkv + ((size_t)b * s_pad + t0) * ld3 + 2 * dim + h * 64;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int f = tid + 256 * it, i = f >> 4, dq = f & 15;
    const float4 v = *reinterpret_cast<const float4*>(src + (size_t)i * ld3 + dq * 4);
    float* d = tile + i * 65 + dq * 4;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  __syncthreads();
  const int d = tid >> 2, part = tid & 3;
  uint32_t hw[8], lw[8];
#pragma unroll
  for (int n = 0; n < 8; ++n)
    split_pair(tile[(part * 16 + 2 * n) * 65 + d], tile[(part * 16 + 2 * n + 1) * 65 + d], hw[n], lw[n]);
  const size_t o = ((size_t)(b * heads + h) * 64 + d) * s_pad + t0 + part * 16;
  *reinterpret_cast<uint4*>(vth + o) = make_uint4(hw[0], hw[1], hw[2], hw[3]);
  *reinterpret_cast<uint4*>(vth + o + 8) = make_uint4(hw[4], hw[5], hw[6], hw[7]);
  *reinterpret_cast<uint4*>(vtl + o) = make_uint4(lw[0], lw[1], lw[2], lw[3]);
  *reinterpret_cast<uint4*>(vtl + o + 8) = make_uint4(lw[4], lw[5], lw[6], lw[7]);
}

// schedule mask of attention_kernel_v2 (see its header).  15 = k-step-major S, accumulator-major P.V, no per-tile max tree,
// loop unrolled by two: 874-893 us against 908-928 us for mask 0 at 110 views (profiles/r03/r03i).  The product library
// instantiates mask 15 only; lab builds select others with dvt_tune_set(1, -510 - mask).
int g_vit_attn_mask = 15;
// dvt_tune_set(1, -531) (default) / (1, -530): dvt_vit_forward's qkv GEMM writes q * log2(e) / 8 and the attention kernel works
// in the log2 domain (attention_v2_body, VAR bit 32) / q as it is and the round-3..5 kernel
int g_vit_attn_log2q = 1;
constexpr int ATT_L2_VAR = 559;  // schedule mask of the log2-domain attention kernel the product launches (attention_v2_body)

#ifdef DVT_LAB
#include "lab/dvt_vit_lab_attn.inc"  // the round-2 kernel, the other schedule masks' dispatch (lab_launch_attention*), lab_attn_tune
#endif

}  // namespace

// Attention's share of dvt_tune_set(1, v) (dvt_vit_tune, dvt_vit.hip)
int vit_attn_tune(int v) {
  if (v == -530 || v == -531) {  // bf16 extractor: attention on q as it is (-530) / on q pre-scaled by log2(e) / 8 (-531, default)
    g_vit_attn_log2q = v == -531;
    return 0;
  }
#ifdef DVT_LAB
  if (const int rc = lab_attn_tune(v); rc != VIT_TUNE_NOT_MINE) return rc;  // (the other kernels and schedule masks)
#endif
  if (v == -502 || v == -510 - 15) return 0;  // the one attention kernel / schedule mask the product library contains
  return VIT_TUNE_NOT_MINE;
}

bool vit_attn_q_prescaled() {
  bool log2q = g_vit_attn_log2q != 0;
#ifdef DVT_LAB
  log2q = log2q && lab_attn_product_selected();  // (the superseded kernels and schedule masks take q as it is)
#endif
  return log2q;
}

// q pre-scaled by log2(e) / 8 (see attention_v2_body, VAR bit 32): the kernel dvt_vit_forward launches since round 6
extern "C" int dvt_vit_attention_log2q(const void* qk, const void* vt, void* out, int batch, int heads,
                                       int s_pad, int n_valid, void* stream) {
  if (!qk || !vt || !out || batch <= 0 || heads <= 0 || s_pad % 16 || n_valid <= 0 || n_valid > s_pad)
    return DVT_E_BADARG;
  DvtProbeScope probe(DVT_PROBE_VIT_ATTN, (hipStream_t)stream,
                      4.0 * (double)n_valid * n_valid * 64.0 * heads * batch);
  const dim3 grid(((s_pad + ATT_Q - 1) / ATT_Q) * heads * batch);
#ifdef DVT_LAB
  if (int rc = 0; lab_launch_attention_l2(qk, vt, out, heads, s_pad, n_valid, grid, (hipStream_t)stream, &rc)) return rc;
#endif
  hipLaunchKernelGGL(attention_kernel_l2<ATT_L2_VAR>, grid, dim3(512), 0, (hipStream_t)stream, (const bf16_t*)qk,
                     (const bf16_t*)vt, (bf16_t*)out, heads, s_pad, n_valid);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int dvt_vit_attention(const void* qk, const void* vt, void* out, int batch, int heads,
                                 int s_pad, int n_valid, void* stream) {
  if (!qk || !vt || !out || batch <= 0 || heads <= 0 || s_pad % 16 || n_valid <= 0 || n_valid > s_pad)
    return DVT_E_BADARG;
  DvtProbeScope probe(DVT_PROBE_VIT_ATTN, (hipStream_t)stream,
                      4.0 * (double)n_valid * n_valid * 64.0 * heads * batch);
  const dim3 grid(((s_pad + ATT_Q - 1) / ATT_Q) * heads * batch);
#ifdef DVT_LAB
  if (int rc = 0; lab_launch_attention(qk, vt, out, heads, s_pad, n_valid, grid, (hipStream_t)stream, &rc)) return rc;
#endif
  hipLaunchKernelGGL(attention_kernel_v2<15>, grid, dim3(512), 0, (hipStream_t)stream, (const bf16_t*)qk,
                     (const bf16_t*)vt, (bf16_t*)out, heads, s_pad, n_valid);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t dvt_vit_attention_x3_scratch_bytes(int batch, int heads, int s_pad) {
  if (batch <= 0 || heads <= 0 || s_pad <= 0) return -1;
  return x3_scratch(batch, heads, s_pad).total * 2;
}

extern "C" int dvt_vit_attention_x3_presplit(const void* scratch, void* out, int batch, int heads, int s_pad, int n_valid,
                                             int split_out, void* stream) {
  if (!out || !scratch || batch <= 0 || heads <= 0 || s_pad % ATT_Q || n_valid <= 0 || n_valid > s_pad)
    return DVT_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const X3Scratch L = x3_scratch(batch, heads, s_pad);
  const bf16_t* qh = (const bf16_t*)scratch;
  const bf16_t* ql = qh + L.ql;
  const bf16_t* vh = qh + L.vh;
  const bf16_t* vl = qh + L.vl;
  DvtProbeScope probe(DVT_PROBE_VIT_ATTN, s, 3.0 * 4.0 * (double)n_valid * n_valid * 64.0 * heads * batch);
  hipLaunchKernelGGL(attention_kernel_v2_x3, dim3((s_pad / ATT_Q) * heads * batch), dim3(512), 0, s,
                     (const bf16_t*)qh, (const bf16_t*)vh, (bf16_t*)out, heads, s_pad, n_valid, (const bf16_t*)ql,
                     (const bf16_t*)vl, split_out);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int dvt_vit_attention_x3(const float* qkv, float* out, void* scratch, int batch, int heads, int s_pad,
                                    int n_valid, void* stream) {
  if (!qkv || !out || !scratch || batch <= 0 || heads <= 0 || s_pad % ATT_Q || n_valid <= 0 || n_valid > s_pad)
    return DVT_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const int dim = heads * 64;
  const long long T = (long long)batch * s_pad;
  const X3Scratch L = x3_scratch(batch, heads, s_pad);
  bf16_t* qh = (bf16_t*)scratch;
  bf16_t* ql = qh + L.ql;
  bf16_t* vh = qh + L.vh;
  bf16_t* vl = qh + L.vl;
  const long long nq = T * (2 * dim / 4);
  hipLaunchKernelGGL(qk_split_kernel, dim3((unsigned)(nq / 256 + 1 < 4096 ? nq / 256 + 1 : 4096)), dim3(256), 0, s, qkv, qh,
                     ql, nq, 2 * dim / 4, 3 * dim);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(v_split_transpose_kernel, dim3(s_pad / 64, heads, batch), dim3(256), 0, s, qkv, vh, vl, heads, s_pad);
  DVT_CHECK_LAUNCH();
  return dvt_vit_attention_x3_presplit(scratch, out, batch, heads, s_pad, n_valid, 0, stream);
}
