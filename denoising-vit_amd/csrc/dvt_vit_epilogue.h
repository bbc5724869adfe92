// dvt_vit_epilogue.h -- the fused epilogues of the bf16 GEMM kernels.  Device code only, no kernel: included by
// dvt_vit_gemm.hip alone (and through it by the developer build's kernels of lab/), held against fp64 one by one by
// tests/test_gpu_vit_epilogues.py.
//   gemm_epilogue<EPI>            from the accumulator registers: the 128 x 128 kernel (gemm_bf16_kernel)
//   gemm_epilogue_lds<EPI, NI>    through a wave's LDS block, row-wise stores: the 256 x 128 ping-pong kernel
//                                 (gemm_bf16_kernel_pp) and the 256 x 256 8-phase kernel (gemm_bf16_kernel_8p) for every
//                                 epilogue but the residual one; the consumer side of the folded LayerNorm lives here
//   gemm_epilogue_resid_sq        LayerScale + residual on a wave's 128 x 64 block of the 8-phase kernel, with the producer
//                                 side of the folded LayerNorm (xb, st_part) and the cache-policy forms of its streams
//   ln_fold                       the folded LayerNorm's fix-up of the accumulators (register form)
//   gelu_erf / gelu_erf_pair      the GELU of the fc1 epilogues (silu_log2, which swiglu_act_kernel shares: dvt_vit_dev.h)
//   NextTilePf                    L2 prefetch for the next workgroup of the XCD (off by default, measured null)
#pragma once
#include "dvt_vit_dev.h"

namespace {

// GELU(x) = 0.5 x (1 + erf(x / sqrt 2)) (nn.GELU(), timm Mlp) = max(x, 0) - 0.5 |x| E(|x|), E = erfc(|x| / sqrt 2).
// Round 5: E by Abramowitz-Stegun 7.1.28, erfc(z) = (1 + a1 z + ... + a6 z^6)^-16 (|abs err| <= 3e-7; measured in fp32
// against fp64: 7.1e-7 on gelu over [-12, 12], i.e. fp32 rounding at |x| ~ 4, far below the bf16 rounding of the output), with
// the powers of 1 / sqrt 2 folded into the coefficients: 6 FMAs + 4 squarings + ONE v_rcp_f32.  Rounds 1-4 used 7.1.26
// (1.5e-7): one v_rcp_f32 AND one v_exp_f32 + 9 FMAs; transcendentals issue at a quarter of the FMA rate and the fc1
// epilogue is VALU-bound (96 of its ~120 cycles per element-wave were this function).  Overflow: the 16th power reaches inf
// beyond |x| ~ 27, v_rcp_f32(inf) = 0, the result is max(x, 0) exactly.  (libm's erff costs ~45 instructions.)
__device__ __forceinline__ float gelu_erf(float x) {
  const float ax = fabsf(x);
  float p = fmaf(ax, 5.3829749049e-06f, 4.8890637117e-05f);
  p = fmaf(p, ax, 3.8003574446e-05f);
  p = fmaf(p, ax, 3.2776263542e-03f);
  p = fmaf(p, ax, 2.1141005680e-02f);
  p = fmaf(p, ax, 4.9867346883e-02f);
  p = fmaf(p, ax, 1.0f);
  p *= p;
  p *= p;
  p *= p;
  p *= p;
  const float e = __builtin_amdgcn_rcpf(p);
  return fmaf(-0.5f * ax, e, fmaxf(x, 0.f));
}

// Two elements at a time on the packed-fp32 pipe (v_pk_fma_f32 / v_pk_mul_f32: both halves are IEEE fma / mul, so every
// result is bit-identical to gelu_erf for non-denormal x).  The compiler packs the LayerNorm affine in front of it by itself but leaves the
// polynomial scalar; written as 2-vectors it is 17 VALU issues per PAIR (2 v_and for |x| -- VOP3P has no abs modifier --, 13
// packed, 2 v_rcp_f32) instead of 30 (15 per element: fmaxf also canonicalises its operand).
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void gelu_erf_pair(float& x0, float& x1) {
  const f32x2_t ax = {fabsf(x0), fabsf(x1)};
  const auto k = [](float c) { return (f32x2_t){c, c}; };
  f32x2_t p = __builtin_elementwise_fma(ax, k(5.3829749049e-06f), k(4.8890637117e-05f));
  p = __builtin_elementwise_fma(p, ax, k(3.8003574446e-05f));
  p = __builtin_elementwise_fma(p, ax, k(3.2776263542e-03f));
  p = __builtin_elementwise_fma(p, ax, k(2.1141005680e-02f));
  p = __builtin_elementwise_fma(p, ax, k(4.9867346883e-02f));
  p = __builtin_elementwise_fma(p, ax, k(1.0f));
  p *= p;
  p *= p;
  p *= p;
  p *= p;
  const f32x2_t e = {__builtin_amdgcn_rcpf(p.x), __builtin_amdgcn_rcpf(p.y)};
  // max(x, 0) = 0.5 x + 0.5 |x| EXACTLY for every x whose half is representable (all normal numbers >= 2^-125, +-0, +inf;
  // tests/test_kernel_math_cpu.py): one packed FMA with a neg modifier instead of two v_max_f32 per element (fmaxf
  // canonicalises its operand first).  A denormal x may lose its last bit (<= 2^-149), far below the bf16 store.
  const f32x2_t xv = {x0, x1};
  const f32x2_t mh = ax * k(-0.5f);
  const f32x2_t pos = __builtin_elementwise_fma(xv, k(0.5f), -mh);
  const f32x2_t r = __builtin_elementwise_fma(mh, e, pos);
  x0 = r.x;
  x1 = r.y;
}

// Fused epilogues.  acc[i][j][r] = C[m0 + wm*64 + i*16 + 4*(lane>>4) + r][n0 + wn*64 + j*16 + (lane&15)]
template <int EPI>
__device__ __forceinline__ void gemm_epilogue(const GemmBArgs& p, f32x4 (&acc)[4][4], int m0, int n0,
                                              int wm, int wn, int lane) {
  const int g = lane >> 4, lc = lane & 15;
  if constexpr (EPI == EPI_SWIGLU) {
    // packed columns: acc[i][j] (j = 0, 1) are the gates of hidden units hb + j * 16 + lc, acc[i][j + 2] their values
    const int ldo = p.N >> 1, hb = (n0 + wn * 64) >> 1;
    const bool odd = lane & 1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 64 + j * 16 + lc, h = hb + j * 16 + lc;
      const float bg = p.bias != nullptr ? p.bias[n] : 0.f, bv = p.bias != nullptr ? p.bias[n + 32] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int mrow = m0 + wm * 64 + i * 16 + 4 * g;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = silu_log2(acc[i][j][r] + bg) * (acc[i][j + 2][r] + bv);
#pragma unroll
        for (int rp = 0; rp < 2; ++rp) {  // column pairs across lanes (l, l ^ 1), as the bf16 stores below
          const float mine0 = v[rp], mine1 = v[rp + 2];
          const float recv = __shfl_xor(odd ? mine0 : mine1, 1, 64);
          const int r = odd ? rp + 2 : rp;
          const uint32_t w = odd ? pack2(recv, mine1) : pack2(mine0, recv);
          *reinterpret_cast<uint32_t*>(p.out + (size_t)(mrow + r) * ldo + (odd ? h - 1 : h)) = w;
        }
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wn * 64 + j * 16 + lc;
    const float bias = p.bias != nullptr ? p.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int mrow = m0 + wm * 64 + i * 16 + 4 * g;  // first of this lane's 4 rows
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r] + bias;
      if (EPI == EPI_QKV && p.q_scale != 0.f && n < p.dim) {  // q columns for the log2-domain attention kernel (tile-uniform)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] *= p.q_scale;
      }
      if (EPI == EPI_RESID) {
        const float gm = p.gamma[n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float* px = p.x + (size_t)(mrow + r) * p.N + n;
          *px = *px + gm * v[r];
        }
      } else if (EPI == EPI_EMBED) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = mrow + r, s = t % p.s_pad;
          float o;
          if (s < p.n_prefix)
            o = p.cls[(size_t)s * p.N + n] + ((p.pos_has_cls && s == 0) ? p.pos[n] : 0.f);
          else if (s < p.n_tokens)
            o = v[r] + p.pos[(size_t)(s - p.n_prefix + p.pos_has_cls) * p.N + n];
          else
            o = 0.f;
          p.x[(size_t)t * p.N + n] = o;
        }
      } else if (EPI == EPI_F32) {
#pragma unroll
        for (int r = 0; r < 4; ++r) p.x[(size_t)(mrow + r) * p.N + n] = v[r];
      } else if (IS_QKV(EPI) && n0 >= 2 * p.dim) {
        // V: transposed store vt[b][h][d][s], the lane's 4 rows are 4 consecutive tokens
        // (a phantom row stores no V^T: vt_rows % 4 == 0, so a lane's 4 rows are all real or all phantom)
        if (mrow >= p.vt_rows) continue;
        const int f = n - 2 * p.dim, h = f >> 6, d = f & 63;
        const int b = mrow / p.s_pad, s = mrow - b * p.s_pad;
        uint2 pk;
        pk.x = pack2(v[0], v[1]);
        pk.y = pack2(v[2], v[3]);
        *reinterpret_cast<uint2*>(p.vt + ((size_t)(b * p.heads + h) * 64 + d) * p.s_pad + s) = pk;
        if (EPI == EPI_QKV_X3) {
          uint2 pl;
          pl.x = pack2(v[0] - __uint_as_float(pk.x << 16), v[1] - __uint_as_float(pk.x & 0xffff0000u));
          pl.y = pack2(v[2] - __uint_as_float(pk.y << 16), v[3] - __uint_as_float(pk.y & 0xffff0000u));
          *reinterpret_cast<uint2*>(p.vt_lo + ((size_t)(b * p.heads + h) * 64 + d) * p.s_pad + s) = pl;
        }
      } else {
        if (IS_GELU(EPI)) {
          gelu_erf_pair(v[0], v[1]);
          gelu_erf_pair(v[2], v[3]);
        }
        const int ldo = (IS_QKV(EPI)) ? 2 * p.dim : p.N;
        // pair adjacent columns across lanes (l, l^1): even lanes store rows r=0,1 of the
        // column pair, odd lanes rows r=2,3 -> 4-B stores instead of 2-B stores
        const bool odd = lane & 1;
#pragma unroll
        for (int rp = 0; rp < 2; ++rp) {
          const float mine0 = v[rp], mine1 = v[rp + 2];
          const float send = odd ? mine0 : mine1;
          const float recv = __shfl_xor(send, 1, 64);
          const int r = odd ? rp + 2 : rp;
          const uint32_t w = odd ? pack2(recv, mine1) : pack2(mine0, recv);
          const int ncol = odd ? n - 1 : n;
          *reinterpret_cast<uint32_t*>(p.out + (size_t)(mrow + r) * ldo + ncol) = w;
        }
      }
    }
  }
}

// ---- LDS-staged epilogue of the 256x128 kernel ---------------------------------------------
// The accumulator layout gives every lane 4 rows x 1 column per 16x16 tile, i.e. 4-byte
// global accesses in 64-B segments (measured: the K=768 proj GEMM spent 630 us where its MFMA
// work is 85 us).  Each wave therefore parks its 64x64 fp32 block (+bias) in its own LDS
// region (stride 68 floats) and reads it back row-wise: fp32 outputs move as float4 (a
// 256-B row segment per 16 lanes), bf16 outputs as 8 columns = 16 B per lane.
constexpr int EP_LD = 68;                      // floats per row of a wave's LDS block
constexpr int EP_WAVE_BYTES = 64 * EP_LD * 4;  // 17408 B x 8 waves = 136 KB <= 144 KB

template <int NI>
__device__ __forceinline__ void ln_fold(const GemmBArgs& p, f32x4 (&acc)[NI][4], int mrow0, int ncol0, int lane);

// L2 prefetch for the NEXT workgroup of this XCD (round 6).  A 256 x 256 tile starts cold: its first LDS-DMAs miss the L2 and a
// K = 768 tile waits ~2.3 us for them while every CU loads at once (profiles/r06/r06j_*: prologue 3.0 us of 25.2).  Workgroups go
// round-robin to the XCDs, so tile blockIdx + 256 is walked by a workgroup of THIS XCD (this L2) about when this one exits: late in
// its epilogue a workgroup touches the first one or two k-tiles' operand lines of that tile -- one dword per 128-B line and thread,
// 256 A rows + 256 W rows.  Placement: program order behind the last load whose result the epilogue still waits for (gfx9 retires
// vector-memory operations of a wave in issue order, and hipcc's counted s_waitcnt does not know these loads: older ones would be
// waited for).  The destination registers stay reserved to the kernel's end (pf_retire): the data lands long after the asm
// statement, and a "dead" destination would be handed out again -- as an address register, the first cut of this faulted.
// MEASURED NULL (profiles/r06/r07a_*, r06z_*): the prologue shrinks as predicted (qkv 3.1 -> 1.1 us, proj 2.5 -> 1.4, fc2 2.4 -> 1.6) and
// the first k-tiles run faster, but the launch does not get shorter (qkv 1793 -> 1812 us, fc1 2786 -> 2769, proj 946 -> 981):
// s_endpgm waits for a wave's outstanding loads, so the fetch latency moves from the next workgroup's prologue into this one's
// exit, and the K = 768 launches are bound by the THROUGHPUT of the shared L2 -> LDS / memory-side path, which a prefetch does
// not add to (the same reason the persistent and staggered variants gave nothing).  Off by default; kept as a knob.
struct NextTilePf {
  const bf16_t* src;  // this thread's operand row of the next tile (nullptr: nothing to touch)
  int n;              // k-tiles to touch (1..2)
  unsigned d0, d1;
};
__device__ __forceinline__ void pf_issue(NextTilePf& f) {
  if (f.src == nullptr) return;
  asm volatile("global_load_dword %0, %1, off" : "=v"(f.d0) : "v"(f.src) : "memory");
  if (f.n > 1) asm volatile("global_load_dword %0, %1, off offset:128" : "=v"(f.d1) : "v"(f.src) : "memory");
}
__device__ __forceinline__ void pf_retire(NextTilePf& f) {
  if (f.src == nullptr) return;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("" ::"v"(f.d0), "v"(f.d1));
}

// NI: 16-row blocks per call (4: a wave's 64 x 64 block, 17 KB of LDS; 2: 32 x 64, 8.5 KB -- the persistent kernel's passes,
// which leave half of the ring to the next tile's operands); `blk0` overrides the wave's LDS block (default: smem + wave *
// EP_WAVE_BYTES)
template <int EPI, int NI = 4, bool OUT_SC1 = false>
__device__ __forceinline__ void gemm_epilogue_lds(const GemmBArgs& p, f32x4 (&acc)[NI][4], int m0,
                                                  int n0, int wm, int wn, int wave, int lane,
                                                  char* smem, char* blk0 = nullptr, NextTilePf* pf = nullptr) {
  static_assert(NI == 4 || NI == 2, "64- or 32-row passes");
  constexpr int ROWS = NI * 16;
  const int g = lane >> 4, lc = lane & 15;
  // LayerNorm folded into this GEMM (see ln_fold): the accumulators are x . W'^T of the UN-normalised rows
  const bool ln = (IS_QKV(EPI) || IS_GELU(EPI) || EPI == EPI_SWIGLU) && p.ln_stats != nullptr;
  float* blk = reinterpret_cast<float*>(blk0 != nullptr ? blk0 : smem + wave * EP_WAVE_BYTES);
  const int nb = n0 + wn * 64;
  if (IS_QKV(EPI) && n0 >= 2 * p.dim) {
    // V tiles: vt[b][h][d][s] wants the TOKENS contiguous.  Round 5: the block goes through LDS transposed -- image
    // [64 features d][64 tokens] (pitch EP_LD), written as ONE ds_write_b128 per accumulator tuple (a lane's 4 rows are 4
    // consecutive tokens of one feature), read back as 8 tokens per lane and stored as 16 B per lane, 8 lanes = one whole
    // 128-B line of a feature row.  Before, every lane stored its tuples straight from the accumulators as 8-byte pieces (64
    // store instructions per block on 32-B segments) behind 32 scattered (mean, rstd) loads: a V tile's epilogue took ~15 us
    // against 3.6 us for a q / k tile, i.e. the qkv GEMM paid +4 us per tile on average (profiles/r05/README.md).
    const int mbv = m0 + wm * 64;
    // NI = 4: 8 chunks of 8 tokens x 8 features per pass, 8 passes; NI = 2: 4 chunks x 16 features, 4 passes
    constexpr int TCH = ROWS / 8, FPP = 64 / TCH, NPASS = 64 / FPP;
    const int tc = lane & (TCH - 1), dl = lane / TCH;  // 8-token chunk of the block, feature within a pass
    // folded LayerNorm: (mean, rstd) of this lane's 8 tokens -- 64 B per lane, coalesced, requested before the LDS traffic
    float4 stq[4];
    float csd[NPASS], bfd[NPASS];  // ... and the column sums / biases of its features (one per pass)
    if (ln) {
      const float4* sp = reinterpret_cast<const float4*>(p.ln_stats + mbv + tc * 8);
#pragma unroll
      for (int q = 0; q < 4; ++q) stq[q] = sp[q];
#pragma unroll
      for (int it = 0; it < NPASS; ++it) {
        csd[it] = p.ln_cs[nb + it * FPP + dl];
        bfd[it] = p.bias[nb + it * FPP + dl];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float bias = (p.bias != nullptr && !ln) ? p.bias[nb + j * 16 + lc] : 0.f;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const float4 t4 = make_float4(acc[i][j][0] + bias, acc[i][j][1] + bias, acc[i][j][2] + bias, acc[i][j][3] + bias);
        *reinterpret_cast<float4*>(blk + (j * 16 + lc) * EP_LD + i * 16 + 4 * g) = t4;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // each wave re-reads its own block only
    const int f0 = nb - 2 * p.dim, hh = f0 >> 6;        // (the block is one head's 64 features: dim_ok_sq / 64-aligned)
    // the image of THIS lane's 8 tokens: a block may straddle two images (s_pad % 64 != 0), an 8-token chunk never (s_pad % 8 == 0);
    // a chunk of phantom rows (at or behind vt_rows, also a multiple of 8) stores nothing -- its image would lie behind `vt`
    const int trow = mbv + tc * 8, bimg = trow / p.s_pad, s0 = trow - bimg * p.s_pad;
    const bool vst = trow < p.vt_rows;
    bf16_t* const vrow = p.vt + ((size_t)(bimg * p.heads + hh) * 64) * p.s_pad + s0;
#pragma unroll
    for (int it = 0; it < NPASS; ++it) {
      if (pf != nullptr && it == 1) pf_issue(*pf);  // (behind the pass that consumed the last loaded parameters)
      const int d = it * FPP + dl;
      const float4 a = *reinterpret_cast<const float4*>(blk + d * EP_LD + tc * 8);
      const float4 b = *reinterpret_cast<const float4*>(blk + d * EP_LD + tc * 8 + 4);
      float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      if (ln) {  // rstd * (acc - mean * cs) + b'
        const float cs = csd[it], bf = bfd[it];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          v[2 * q] = fmaf(stq[q].y, v[2 * q] - stq[q].x * cs, bf);
          v[2 * q + 1] = fmaf(stq[q].w, v[2 * q + 1] - stq[q].z * cs, bf);
        }
      }
      typedef unsigned u32x4v_t __attribute__((ext_vector_type(4)));
      const u32x4v_t hi = {pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
      if (vst) {
        u32x4v_t* vdst = reinterpret_cast<u32x4v_t*>(vrow + (size_t)d * p.s_pad);
        if (EPI == EPI_QKV && p.nt_store)
          __builtin_nontemporal_store(hi, vdst);
        else
          *vdst = hi;
      }
      if constexpr (EPI == EPI_QKV_X3) {
        u32x4v_t lo;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          lo[q] = pack2(v[2 * q] - __uint_as_float(hi[q] << 16), v[2 * q + 1] - __uint_as_float(hi[q] & 0xffff0000u));
        if (vst) *reinterpret_cast<u32x4v_t*>(p.vt_lo + (vrow - p.vt) + (size_t)d * p.s_pad) = lo;
      }
    }
    return;
  }
  // (mean, rstd) of the block's 64 rows: ONE coalesced load per lane, requested now and parked in the padding
  // columns of the LDS block with the accumulators (as 32 loads per lane at the top of the epilogue they cost a full
  // memory latency per tile)
  float2 st_row = make_float2(0.f, 0.f);
  if (ln && lane < ROWS) st_row = p.ln_stats[m0 + wm * 64 + lane];
  // ... and so are the folded LayerNorm's column sums / biases of the lane's 8 output columns (round 5; before, they were
  // requested after the LDS round trip, right in front of the loop that needs them.  Same-box A/B: no difference -- the other
  // waves of the CU cover that latency -- kept here because it is the natural place)
  const int c8_ln = (lane & 7) * 8;
  float4 cs0 = make_float4(0.f, 0.f, 0.f, 0.f), cs1 = cs0, bf0 = cs0, bf1 = cs0;
  if (ln && EPI != EPI_RESID && EPI != EPI_EMBED && EPI != EPI_F32 && EPI != EPI_SWIGLU) {
    cs0 = *reinterpret_cast<const float4*>(p.ln_cs + nb + c8_ln);
    cs1 = *reinterpret_cast<const float4*>(p.ln_cs + nb + c8_ln + 4);
    bf0 = *reinterpret_cast<const float4*>(p.bias + nb + c8_ln);
    bf1 = *reinterpret_cast<const float4*>(p.bias + nb + c8_ln + 4);
  }
#ifdef DVT_LAB
  if (!(p.abl & 1))
#endif
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float bias = (p.bias != nullptr && !ln) ? p.bias[nb + j * 16 + lc] : 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) blk[(i * 16 + 4 * g + r) * EP_LD + j * 16 + lc] = acc[i][j][r] + bias;
  }
  if (ln && lane < ROWS) *reinterpret_cast<float2*>(blk + lane * EP_LD + 64) = st_row;
  // each wave only re-reads its own block: no workgroup barrier needed, only LDS completion
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const int mb = m0 + wm * 64;
  if constexpr (EPI == EPI_SWIGLU) {
    // The block's columns are packed: [0, 32) gates, [32, 64) the values of the same 32 hidden units (nb / 2 ...).  A lane
    // takes 8 units of one row -- 8 gates + 8 values out of LDS, 16 B of bf16 out; 4 lanes = the block's 64-B share of an
    // output row (the wave next door, wn + 1, writes the other half of the 128-B line), 16 rows per pass.  The 16 lanes of a
    // quarter wave read rows {0, 1, 8, 9} + 2 q of the pass: at the pitch of 68 floats rows two apart would share banks.
    const int c8 = (lane & 3) * 8, ldo = p.N >> 1;
    const int rsub = ((lane >> 2) & 1) + 8 * ((lane >> 3) & 1) + 2 * (lane >> 4);
    alignas(16) float csg[8], csv[8], bfg[8], bfv[8];
    if (ln) {
#pragma unroll
      for (int q = 0; q < 8; q += 4) {
        *reinterpret_cast<float4*>(csg + q) = *reinterpret_cast<const float4*>(p.ln_cs + nb + c8 + q);
        *reinterpret_cast<float4*>(csv + q) = *reinterpret_cast<const float4*>(p.ln_cs + nb + 32 + c8 + q);
        *reinterpret_cast<float4*>(bfg + q) = *reinterpret_cast<const float4*>(p.bias + nb + c8 + q);
        *reinterpret_cast<float4*>(bfv + q) = *reinterpret_cast<const float4*>(p.bias + nb + 32 + c8 + q);
      }
    }
#pragma unroll 1
    for (int it = 0; it < ROWS / 16; ++it) {
      if (pf != nullptr && it == 1) pf_issue(*pf);
      const int row = it * 16 + rsub;
      alignas(16) float gt[8], vl[8];
#pragma unroll
      for (int q = 0; q < 8; q += 4) {
        *reinterpret_cast<float4*>(gt + q) = *reinterpret_cast<const float4*>(blk + row * EP_LD + c8 + q);
        *reinterpret_cast<float4*>(vl + q) = *reinterpret_cast<const float4*>(blk + row * EP_LD + 32 + c8 + q);
      }
      if (ln) {  // rstd * (acc - mean * cs) + b' on both halves
        const float2 stv = *reinterpret_cast<const float2*>(blk + row * EP_LD + 64);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          gt[q] = fmaf(stv.y, gt[q] - stv.x * csg[q], bfg[q]);
          vl[q] = fmaf(stv.y, vl[q] - stv.x * csv[q], bfv[q]);
        }
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) gt[q] = silu_log2(gt[q]) * vl[q];
      typedef unsigned u32x4s_t __attribute__((ext_vector_type(4)));
      const u32x4s_t val = {pack2(gt[0], gt[1]), pack2(gt[2], gt[3]), pack2(gt[4], gt[5]), pack2(gt[6], gt[7])};
      u32x4s_t* dst = reinterpret_cast<u32x4s_t*>(p.out + (size_t)(mb + row) * ldo + (nb >> 1) + c8);
      if (p.nt_store)
        __builtin_nontemporal_store(val, dst);
      else
        *dst = val;
    }
    return;
  }
  if (EPI == EPI_RESID || EPI == EPI_EMBED || EPI == EPI_F32) {
    const int c4 = lc * 4;  // 16 lanes x float4 = one 64-float row; 4 rows per pass
    float4 gm = make_float4(1.f, 1.f, 1.f, 1.f);
    if (EPI == EPI_RESID) gm = *reinterpret_cast<const float4*>(p.gamma + nb + c4);
#pragma unroll 4
    for (int it = 0; it < ROWS / 4; ++it) {
      const int row = it * 4 + g;
      if (pf != nullptr && it == ROWS / 8 && EPI == EPI_F32) pf_issue(*pf);  // (EPI_F32 loads nothing per row; the others do)
      const float4 v = *reinterpret_cast<const float4*>(blk + row * EP_LD + c4);
      const int t = mb + row;
      float4* px = reinterpret_cast<float4*>(p.x + (size_t)t * p.N + nb + c4);
      if (EPI == EPI_RESID) {
        float4 o = *px;
        o.x += gm.x * v.x;
        o.y += gm.y * v.y;
        o.z += gm.z * v.z;
        o.w += gm.w * v.w;
        *px = o;
      } else if (EPI == EPI_F32) {
        *px = v;
      } else {
        const int sidx = t % p.s_pad;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (sidx < p.n_prefix) {  // cls / register tokens (timm: cls gets pos_embed[0] unless no_embed_class)
          o = *reinterpret_cast<const float4*>(p.cls + (size_t)sidx * p.N + nb + c4);
          if (p.pos_has_cls && sidx == 0) {
            const float4 q = *reinterpret_cast<const float4*>(p.pos + nb + c4);
            o = make_float4(o.x + q.x, o.y + q.y, o.z + q.z, o.w + q.w);
          }
        } else if (sidx < p.n_tokens) {
          const float4 q = *reinterpret_cast<const float4*>(
              p.pos + (size_t)(sidx - p.n_prefix + p.pos_has_cls) * p.N + nb + c4);
          o = make_float4(v.x + q.x, v.y + q.y, v.z + q.z, v.w + q.w);
        }
        *px = o;
      }
    }
  } else {
    const int ldo = (IS_QKV(EPI)) ? 2 * p.dim : p.N;
    const int c8 = (lane & 7) * 8;  // 8 lanes x 8 columns = one row; 8 rows per pass
    const float qsc = (EPI == EPI_QKV && nb < p.dim) ? p.q_scale : 0.f;  // (wave-uniform: a 64-column block is q, k or v)
    // (GELU: one row at a time -- four rows of erf polynomials in flight took the fc1 kernel to 254 VGPRs,
    // and at 2 x 256 registers per SIMD no wave of the fit's streaming kernels can share the CU)
#pragma unroll(IS_GELU(EPI) ? 1 : 4)
    for (int it = 0; it < ROWS / 8; ++it) {
      if (pf != nullptr && it == 1) pf_issue(*pf);  // (pass 0 consumed the last loaded parameters)
      const int row = it * 8 + (lane >> 3);
      float4 a = *reinterpret_cast<const float4*>(blk + row * EP_LD + c8);
      float4 b = *reinterpret_cast<const float4*>(blk + row * EP_LD + c8 + 4);
      if (ln) {  // rstd * (acc - mean * cs) + b'
        const float2 stv = *reinterpret_cast<const float2*>(blk + row * EP_LD + 64);
        const float mu = stv.x, rs = stv.y;
        a.x = fmaf(rs, a.x - mu * cs0.x, bf0.x);
        a.y = fmaf(rs, a.y - mu * cs0.y, bf0.y);
        a.z = fmaf(rs, a.z - mu * cs0.z, bf0.z);
        a.w = fmaf(rs, a.w - mu * cs0.w, bf0.w);
        b.x = fmaf(rs, b.x - mu * cs1.x, bf1.x);
        b.y = fmaf(rs, b.y - mu * cs1.y, bf1.y);
        b.z = fmaf(rs, b.z - mu * cs1.z, bf1.z);
        b.w = fmaf(rs, b.w - mu * cs1.w, bf1.w);
      }
      if (IS_GELU(EPI)) {
        gelu_erf_pair(a.x, a.y);
        gelu_erf_pair(a.z, a.w);
        gelu_erf_pair(b.x, b.y);
        gelu_erf_pair(b.z, b.w);
      }
      if (EPI == EPI_QKV && qsc != 0.f) {  // q columns (tile-uniform): * log2(e) / 8 on the fp32 value, ONE rounding to bf16 as before
        a.x *= qsc; a.y *= qsc; a.z *= qsc; a.w *= qsc;
        b.x *= qsc; b.y *= qsc; b.z *= qsc; b.w *= qsc;
      }
      uint4 pk;
      pk.x = pack2(a.x, a.y);
      pk.y = pack2(a.z, a.w);
      pk.z = pack2(b.x, b.y);
      pk.w = pack2(b.z, b.w);
      typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
      const u32x4_t val = {pk.x, pk.y, pk.z, pk.w};
      if constexpr (IS_X3(EPI)) {
        u32x4_t vlo;
        vlo.x = pack2(a.x - __uint_as_float(pk.x << 16), a.y - __uint_as_float(pk.x & 0xffff0000u));
        vlo.y = pack2(a.z - __uint_as_float(pk.y << 16), a.w - __uint_as_float(pk.y & 0xffff0000u));
        vlo.z = pack2(b.x - __uint_as_float(pk.z << 16), b.y - __uint_as_float(pk.z & 0xffff0000u));
        vlo.w = pack2(b.z - __uint_as_float(pk.w << 16), b.w - __uint_as_float(pk.w & 0xffff0000u));
        if constexpr (EPI == EPI_GELU_X3) {  // the next GEMM's A row: [hi | hi | lo], each N wide
          bf16_t* r3 = p.out + (size_t)(mb + row) * (3 * p.N) + nb + c8;
          *reinterpret_cast<u32x4_t*>(r3) = val;
          *reinterpret_cast<u32x4_t*>(r3 + p.N) = val;
          *reinterpret_cast<u32x4_t*>(r3 + 2 * p.N) = vlo;
        } else {
          *reinterpret_cast<u32x4_t*>(p.out + (size_t)(mb + row) * ldo + nb + c8) = val;
          *reinterpret_cast<u32x4_t*>(p.out_lo + (size_t)(mb + row) * ldo + nb + c8) = vlo;
        }
        continue;
      }
      u32x4_t* dst = reinterpret_cast<u32x4_t*>(p.out + (size_t)(mb + row) * ldo + nb + c8);
      if constexpr (OUT_SC1) {
        // write-through (sc1): the line does not stay in the XCD's L2 behind the store.  A buffer store based at the block,
        // the row offset in the VGPR offset (see RS_ST)
        typedef int i32x4s_t __attribute__((ext_vector_type(4)));
        const __amdgpu_buffer_rsrc_t orc = __builtin_amdgcn_make_buffer_rsrc(p.out + (size_t)mb * ldo + nb, 0, 0x7fffffff, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4s_t, val), orc, (row * ldo + c8) * 2, 0, 16);
      } else if (p.nt_store)
        __builtin_nontemporal_store(val, dst);  // streamed output: meant not to displace the operand panels in L2
      else
        *dst = val;
    }
  }
}

// ---- LayerNorm folded into the neighbouring GEMMs ------------------------------------------------------------
// xn = (x - mu) * rstd * gamma + beta, then xn . W^T + b, is   rstd * (x . W'^T - mu * cs) + b'   with
// W' = gamma (.) W, cs[n] = sum_k W'[n][k], b' = b + W beta.  So the consumer GEMM (qkv, fc1) reads bf16(x)
// itself and fixes its accumulators up with the row's (mu, rstd); the producer (the residual epilogue of proj /
// fc2) writes bf16(x) and per-row partial (sum, sum of squares) next to the fp32 x it writes anyway.  The
// LayerNorm kernel between them -- 553 MB read + 277 MB written per call, 168 calls per image -- disappears.
template <int NI>
__device__ __forceinline__ void ln_fold(const GemmBArgs& p, f32x4 (&acc)[NI][4], int mrow0, int ncol0, int lane) {
  const int g = lane >> 4, lc = lane & 15;
  float cs[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) cs[j] = p.ln_cs[ncol0 + j * 16 + lc];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float2 st = p.ln_stats[mrow0 + i * 16 + 4 * g + r];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j][r] = st.y * (acc[i][j][r] - st.x * cs[j]);
    }
}

// sum over the 16 lanes of a DPP row (rotations inside the row: v_add_f32 with a row_ror modifier, no LDS traffic)
__device__ __forceinline__ float row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));
  return v;
}

// EPI_RESID epilogue of the 256x256 kernels: x[m, n] += gamma[n] * (acc + bias[n]) on a wave's
// 128 x 64 block.  The fp32 residual stream is a read-modify-write of 8 B per element (1.1 GB per
// launch); with the loads issued four at a time inside the row loop a tile's epilogue took 4 x 2
// rounds of memory latency -- longer than the whole K = 768 k-loop.  Here all 16 float4 rows of a
// 64-row half are requested up front (64 VGPRs; the k-loop's fragment registers are dead), and the
// second half's requests go out as soon as the first half's accumulators are parked in LDS.
// LD_AUX / ST_AUX: cache-policy bits (the intrinsics' aux argument: 0 default, 2 = nt, 16 = sc1, write-through) of the fp32
// residual loads / stores; XB_NT: the bf16 xb stores carry the nt hint (launch_gemm picks the 8p kernel's instantiation from
// g_vit_epi_policy; policy only, the values are the same).  The st_part stores (8 B per row and 64 columns, 0.3 % of the
// epilogue's bytes) stay plain: as a second nt form they took the kernel from 230 to 234 VGPRs.
template <int LD_AUX = 0, int ST_AUX = 0, bool XB_NT = false>
__device__ __forceinline__ void gemm_epilogue_resid_sq(const GemmBArgs& p, f32x4 (&acc)[8][4], int mb,
                                                       int nb, int wave, int lane, char* smem, NextTilePf* pf = nullptr) {
  const int g = lane >> 4, lc = lane & 15, c4 = lc * 4;
  float* blk = reinterpret_cast<float*>(smem + wave * EP_WAVE_BYTES);
  // buffer addressing: one resource (SGPRs) based at the block, ONE 32-bit lane offset and a
  // scalar row offset per access -- 32 rows of 64-bit global addresses would cost 64 VGPRs
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      p.x + (size_t)mb * p.N + nb, 0, 0x7fffffff, 0x00020000);
  const int loff = (g * p.N + c4) * 4;
  const int rstep = p.N * 16;  // bytes per 4 rows
  typedef int i32x4_t __attribute__((ext_vector_type(4)));
#define RS_LD(it) __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(xr, loff, (it) * rstep, LD_AUX))
// Stores put the row offset into the VGPR offset (soffset = literal 0): with an SGPR soffset the
// compiler assumes there is no ">64-bit store data overwritten by the next VALU" hazard and emits
// no wait state, but gfx950 showed exactly that corruption (lanes 12-15 of each 16, one dword).
#define RS_ST(it, v) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4_t, v), xr, loff + (it) * rstep, 0, ST_AUX)
// LayerNorm producer side: bf16 copy of the new row piece (16 lanes x 8 B = 128 B per row) and the row's partial
// (sum, sum of squares) over this wave's 64 columns: xor-reduce over the 16 lanes that hold the row
#define RS_LN(it, o)                                                                                    \
  do {                                                                                                  \
    const int row_ = mb + (it) * 4 + g;                                                                 \
    uint2 pk_;                                                                                          \
    pk_.x = pack2((o).x, (o).y);                                                                        \
    pk_.y = pack2((o).z, (o).w);                                                                        \
    uint2* xbp_ = reinterpret_cast<uint2*>(p.xb + (size_t)row_ * p.N + nb + c4);                        \
    if constexpr (XB_NT)                                                                                \
      __builtin_nontemporal_store(__builtin_bit_cast(unsigned long long, pk_),                          \
                                  reinterpret_cast<unsigned long long*>(xbp_));                         \
    else                                                                                                \
      *xbp_ = pk_;                                                                                      \
    float s1_ = ((o).x + (o).y) + ((o).z + (o).w);                                                      \
    float s2_ = ((o).x * (o).x + (o).y * (o).y) + ((o).z * (o).z + (o).w * (o).w);                      \
    s1_ = row16_sum(s1_);                                                                               \
    s2_ = row16_sum(s2_);                                                                               \
    if (lc == 0) p.st_part[(size_t)(nb >> 6) * p.M + row_] = make_float2(s1_, s2_);                     \
  } while (0)
  float4 xl[16], xh[16];
#pragma unroll
  for (int it = 0; it < 16; ++it) xl[it] = RS_LD(it);
  float bias[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bias[j] = p.bias != nullptr ? p.bias[nb + j * 16 + lc] : 0.f;
  const float4 gm = *reinterpret_cast<const float4*>(p.gamma + nb + c4);
#ifdef DVT_LAB
  if (!(p.abl & 1))
#endif
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) blk[(i * 16 + 4 * g + r) * EP_LD + j * 16 + lc] = acc[i][j][r] + bias[j];
#pragma unroll
  for (int it = 0; it < 16; ++it) xh[it] = RS_LD(16 + it);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    const float4 v = *reinterpret_cast<const float4*>(blk + (it * 4 + g) * EP_LD + c4);
    float4 o = xl[it];
    o.x += gm.x * v.x;
    o.y += gm.y * v.y;
    o.z += gm.z * v.z;
    o.w += gm.w * v.w;
    RS_ST(it, o);
    if (p.xb != nullptr) RS_LN(it, o);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // own reads of the block are complete
  if (pf != nullptr) pf_issue(*pf);  // younger than every row load, older than the second half's stores only
#ifdef DVT_LAB
  if (!(p.abl & 1))
#endif
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) blk[(i * 16 + 4 * g + r) * EP_LD + j * 16 + lc] = acc[4 + i][j][r] + bias[j];
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    const float4 v = *reinterpret_cast<const float4*>(blk + (it * 4 + g) * EP_LD + c4);
    float4 o = xh[it];
    o.x += gm.x * v.x;
    o.y += gm.y * v.y;
    o.z += gm.z * v.z;
    o.w += gm.w * v.w;
    RS_ST(16 + it, o);
    if (p.xb != nullptr) RS_LN(16 + it, o);
  }
#undef RS_LD
#undef RS_ST
#undef RS_LN
}

}  // namespace
