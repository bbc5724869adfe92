// The trained transformer block that the stage-2 step (dvt_stage2.hip) and the stage-3 step (dvt_stage3.hip) both run
// (dvt_block_train.h).  Its pieces: the residual add fused with the LayerNorm behind it (plain and LayerScale), LayerNorm and
// LayerScale backward, GELU, the fused attention-row kernels, the loss rows, the linear layers' forward / backward on the
// 128 x 128 x 32 exact-fp32 tile (or, stage 3's opt-in, on the bf16 GEMM), the batched attention products with the attention
// forward / backward launch sequences around them, and the side stream those sequences fork onto.  Then the block itself,
// block_fwd / block_bwd, and the carving of its workspace.  One compiled copy: what tests/test_gpu_parts.py drives through the
// dvt_parts_* forwarders at the end of this file is exactly what both trainers launch.  The A/B switches are the process's,
// defined in dvt_stage2.hip.
#include <map>
#include <mutex>
#include "dvt_block_train.h"
#include "dvt_row_dev.h"
#include "../../include/dvt_parts.h"
#include "../../include/dvt_stage3.h"

namespace {

// ==========================================================================================================
// (a [+ b]) -> sum, LayerNorm(sum) -> xn, per-row mean / rstd.  One wave per row.
//   a: packed [batch, T, C] (a_packed) or padded [R, C];  b: nullptr, pos_embed [T, C] (b_is_pos) or padded [R, C]
// Rows t >= T: sum = xn = 0, mean = rstd = 0.
// online_denoiser.py:88-89 (x + pos_embed), Block: x + attn(norm1(x)), x + mlp(norm2(x)).
// ==========================================================================================================
template <int C>
__global__ __launch_bounds__(256) void s2_add_ln_kernel(const float* __restrict__ a, int a_packed,
                                                        const float* __restrict__ b, int b_is_pos,
                                                        float* __restrict__ sum_out, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ xn,
                                                        float* __restrict__ mean, float* __restrict__ rstd, int T,
                                                        int Tp, int R, float eps) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int img = r / Tp, t = r - img * Tp;
  Row<C> x;
  if (t >= T) {
    x.zero();
    if (sum_out) x.store(sum_out + (size_t)r * C, lane);
    x.store(xn + (size_t)r * C, lane);
    if (lane == 0) {
      mean[r] = 0.f;
      rstd[r] = 0.f;
    }
    return;
  }
  x.load(a_packed ? a + ((size_t)img * T + t) * C : a + (size_t)r * C, lane);
  if (b) {
    Row<C> y;
    y.load(b_is_pos ? b + (size_t)t * C : b + (size_t)r * C, lane);
    ROW_FOR(j, Row<C>::NJ) x.v[j] = f4_add(x.v[j], y.v[j]);
  }
  if (sum_out) x.store(sum_out + (size_t)r * C, lane);
  const float mu = x.sum() * (1.0f / C);
  Row<C> d;
  float ss = 0.f;
  ROW_FOR(j, Row<C>::NJ) {
    const int i = lane + 64 * j;
    d.v[j] = (i < C / 4) ? f4_sub(x.v[j], make_float4(mu, mu, mu, mu)) : make_float4(0.f, 0.f, 0.f, 0.f);
    ss += f4_dot(d.v[j], d.v[j]);
  }
  const float var = wave_sum(ss) * (1.0f / C);
  const float rs = 1.0f / sqrtf(var + eps);
  Row<C> g, be;
  g.load(gamma, lane);
  be.load(beta, lane);
  ROW_FOR(j, Row<C>::NJ) d.v[j] = f4_add(f4_mul(f4_scale(d.v[j], rs), g.v[j]), be.v[j]);
  d.store(xn + (size_t)r * C, lane);
  if (lane == 0) {
    mean[r] = mu;
    rstd[r] = rs;
  }
}

// ==========================================================================================================
// LayerScale residual add fused with the LayerNorm behind it, one wave per row (timm Block: x = x + ls(f(norm(x))), then the
// next block's norm1 or the final norm):  sum = a + ls (.) f,  xn = LayerNorm(sum) * gamma + beta, per-row mean / rstd kept.
// ls == nullptr: sum = a (the first block's norm1).  Rows t >= T: sum = xn = 0, mean = rstd = 0.  LayerNorm arithmetic as
// s2_add_ln_kernel (two passes, 1 / sqrt(var + eps)).
// ==========================================================================================================
template <int C>
__global__ __launch_bounds__(256) void s3_ls_add_ln_kernel(const float* __restrict__ a, const float* __restrict__ f,
                                                           const float* __restrict__ ls, float* __restrict__ sum_out,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ xn, float* __restrict__ mean,
                                                           float* __restrict__ rstd, int T, int Tp, int R, float eps) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int t = r % Tp;
  Row<C> x;
  if (t >= T) {
    x.zero();
    if (sum_out) x.store(sum_out + (size_t)r * C, lane);
    x.store(xn + (size_t)r * C, lane);
    if (lane == 0) {
      mean[r] = 0.f;
      rstd[r] = 0.f;
    }
    return;
  }
  x.load(a + (size_t)r * C, lane);
  if (ls) {
    Row<C> y, g;
    y.load(f + (size_t)r * C, lane);
    g.load(ls, lane);
    ROW_FOR(j, Row<C>::NJ) x.v[j] = f4_add(x.v[j], f4_mul(g.v[j], y.v[j]));
  }
  if (sum_out) x.store(sum_out + (size_t)r * C, lane);
  const float mu = x.sum() * (1.0f / C);
  Row<C> d;
  float ss = 0.f;
  ROW_FOR(j, Row<C>::NJ) {
    const int i = lane + 64 * j;
    d.v[j] = (i < C / 4) ? f4_sub(x.v[j], make_float4(mu, mu, mu, mu)) : make_float4(0.f, 0.f, 0.f, 0.f);
    ss += f4_dot(d.v[j], d.v[j]);
  }
  const float var = wave_sum(ss) * (1.0f / C);
  const float rs = 1.0f / sqrtf(var + eps);
  Row<C> g, be;
  g.load(gamma, lane);
  be.load(beta, lane);
  ROW_FOR(j, Row<C>::NJ) d.v[j] = f4_add(f4_mul(f4_scale(d.v[j], rs), g.v[j]), be.v[j]);
  d.store(xn + (size_t)r * C, lane);
  if (lane == 0) {
    mean[r] = mu;
    rstd[r] = rs;
  }
}

// ==========================================================================================================
// LayerScale backward: y = x + ls (.) f  ->  df = ls (.) dy,  dls += sum_rows f (.) dy  (dx = dy is the caller's residual).
// A 256-thread block walks 32 rows (8 per wave), reduces the 4 waves through LDS and issues one atomic per column, as
// s2_ln_bwd_kernel does.
// ==========================================================================================================
template <int C>
__global__ __launch_bounds__(256) void s3_ls_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ f,
                                                        const float* __restrict__ ls, float* __restrict__ df,
                                                        float* __restrict__ dls, int R) {
  constexpr int NJ = Row<C>::NJ;
  __shared__ float red[4][C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Row<C> g, acc;
  g.load(ls, lane);
  acc.zero();
  const int r0 = blockIdx.x * 32 + wave * 8;
  for (int i = 0; i < 8; ++i) {
    const int r = r0 + i;
    if (r >= R) break;
    Row<C> d, fv;
    d.load(dy + (size_t)r * C, lane);
    fv.load(f + (size_t)r * C, lane);
    ROW_FOR(j, NJ) {
      acc.v[j] = f4_add(acc.v[j], f4_mul(fv.v[j], d.v[j]));
      d.v[j] = f4_mul(g.v[j], d.v[j]);
    }
    d.store(df + (size_t)r * C, lane);
  }
  ROW_FOR(j, NJ) {
    const int idx = lane + 64 * j;
    if (idx < C / 4) *reinterpret_cast<float4*>(&red[wave][4 * idx]) = acc.v[j];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) atomic_add_f32(dls + c, (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]));
}

// ==========================================================================================================
// LayerNorm backward fused with the residual-path gradient:
//   dx = dres + rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)),  g = dy * gamma,  xhat = (x - mean) * rstd
//   dgamma += sum_rows dy * xhat,  dbeta += sum_rows dy
// A 256-thread block walks 32 rows (8 per wave), keeps the parameter-gradient partials in registers, reduces
// the 4 waves through LDS and issues ONE atomic per column.
// ==========================================================================================================
template <int C>
__global__ __launch_bounds__(256) void s2_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        const float* __restrict__ gamma, const float* __restrict__ dres,
                                                        float* __restrict__ dx, float* __restrict__ dgamma,
                                                        float* __restrict__ dbeta, int R) {
  constexpr int NJ = Row<C>::NJ;
  __shared__ float red[2][4][C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Row<C> gm, ag, ab;
  gm.load(gamma, lane);
  ag.zero();
  ab.zero();
  const int r0 = blockIdx.x * 32 + wave * 8;
  for (int i = 0; i < 8; ++i) {
    const int r = r0 + i;
    if (r >= R) break;
    const float mu = mean[r], rs = rstd[r];
    Row<C> d, xv, o;
    d.load(dy + (size_t)r * C, lane);
    xv.load(x + (size_t)r * C, lane);
    float s1 = 0.f, s2 = 0.f;
    ROW_FOR(j, NJ) {
      const int idx = lane + 64 * j;
      const float4 xh = (idx < C / 4) ? f4_scale(f4_sub(xv.v[j], make_float4(mu, mu, mu, mu)), rs)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 g = f4_mul(d.v[j], gm.v[j]);
      ag.v[j] = f4_add(ag.v[j], f4_mul(d.v[j], xh));
      ab.v[j] = f4_add(ab.v[j], d.v[j]);
      s1 += (g.x + g.y) + (g.z + g.w);
      s2 += f4_dot(g, xh);
      xv.v[j] = xh;
      d.v[j] = g;
    }
    const float m1 = wave_sum(s1) * (1.0f / C), m2 = wave_sum(s2) * (1.0f / C);
    if (dres) o.load(dres + (size_t)r * C, lane); else o.zero();
    ROW_FOR(j, NJ) {
      const float4 t = f4_sub(f4_sub(d.v[j], make_float4(m1, m1, m1, m1)), f4_scale(xv.v[j], m2));
      o.v[j] = f4_add(o.v[j], f4_scale(t, rs));
    }
    o.store(dx + (size_t)r * C, lane);
  }
  ROW_FOR(j, NJ) {
    const int idx = lane + 64 * j;
    if (idx < C / 4) {
      *reinterpret_cast<float4*>(&red[0][wave][4 * idx]) = ag.v[j];
      *reinterpret_cast<float4*>(&red[1][wave][4 * idx]) = ab.v[j];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    atomic_add_f32(dgamma + c, (red[0][0][c] + red[0][1][c]) + (red[0][2][c] + red[0][3][c]));
    atomic_add_f32(dbeta + c, (red[1][0][c] + red[1][1][c]) + (red[1][2][c] + red[1][3][c]));
  }
}

// ==========================================================================================================
// GELU (nn.GELU(), exact erf) forward / backward, elementwise over float4
// ==========================================================================================================
__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_grad_f(float x) {
  const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
  const float pdf = 0.3989422804014327f * __expf(-0.5f * x * x);
  return cdf + x * pdf;
}
__global__ __launch_bounds__(256) void s2_gelu_kernel(const float4* __restrict__ h, float4* __restrict__ a, int64_t n4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 v = h[i];
  a[i] = make_float4(gelu_f(v.x), gelu_f(v.y), gelu_f(v.z), gelu_f(v.w));
}
__global__ __launch_bounds__(256) void s2_gelu_bwd_kernel(const float4* __restrict__ h, float4* __restrict__ da, int64_t n4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 v = h[i], d = da[i];
  da[i] = make_float4(d.x * gelu_grad_f(v.x), d.y * gelu_grad_f(v.y), d.z * gelu_grad_f(v.z), d.w * gelu_grad_f(v.w));
}

// ==========================================================================================================
// Round 6: the two [Tp][Tp]-sized products of a head WITH the softmax arithmetic that used to run over their output.
// One workgroup = 128 query rows of one (image, head): 4 waves x 32 rows, the row operand (q, or d ao) lives in registers
// -- 32 fragment values per lane, as in the fp32 extractor's attention kernel --, the key-side operand (k, or v) streams
// through LDS in 32-key tiles (two buffers, one barrier per tile).  v_mfma_f32_32x32x2_f32 in BOTH operand orders off the
// SAME registers and the same LDS reads:
//   T-order  D = K_tile . A^T   lane holds query (lane & 31), keys kappa(r) + 4 (lane >> 5): row statistics are lane-local
//   N-order  D = A . K_tile^T   lane holds key (lane & 31), queries kappa(r) + 4 (lane >> 5): a half-wave stores 32
//                               consecutive keys of one query row = one whole 128-B line per instruction
// MODE 0, forward (main_denoiser.py:138-140 -> timm Attention.forward: softmax(q k^T / 8)): sweep 1 in T-order forms every
//   query's running max and sum (base 2, the scale folded into q), sweep 2 recomputes the logits in N-order and writes
//   P = 2^(s - m) / l ONCE.  Before: S written by a 64 x 64-tile GEMM (186 k workgroups of 32 MFMAs per wave), read and
//   rewritten by s2_softmax_kernel: 9 GB of traffic, 1.76 + 1.22 ms per step at batch 32.  Padded query rows and key columns
//   (>= T) get P = 0, as s2_softmax_kernel wrote them.
// MODE 1, backward: dS = scale P (.) (dao v^T - D) in N-order, D = rowsum(dP (.) P) = dao . ao from s2_rowdot_kernel; P is
//   read once (requested a tile ahead), dP never exists.
// ==========================================================================================================
constexpr int AR_K = 32, AR_LD = 65;  // odd pitch: the 32 rows of a key-tile fragment read hit 32 banks
typedef float floatx16 __attribute__((ext_vector_type(16)));

template <int MODE>
__global__ __launch_bounds__(256) void s2_attn_rows_kernel(const float* __restrict__ rowop, int ld_row, const float* __restrict__ keyop,
                                                           int ld_key, const float* __restrict__ Pin, const float* __restrict__ D,
                                                           float* __restrict__ out, int heads, int T, int Tp, float scale) {
  __shared__ float Ks[2][AR_K * AR_LD];
  __shared__ float stat[2][AR_Q];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h2 = lane >> 5;
  const int nqb = Tp / AR_Q;
  const int id = blockIdx.x;
  const int qb = id % nqb, hd = (id / nqb) % heads, b = id / (nqb * heads);
  const size_t row0 = (size_t)b * Tp;
  const int q0w = qb * AR_Q + wave * 32;  // first query row of this wave inside the image
  const float LOG2E = 1.4426950408889634f;
  // row-operand fragments of this lane: A[query q0w + j][d = 2 s + h2] (forward: q * scale * log2(e): softmax in base 2)
  float af[32];
  {
    const float* ap = rowop + (row0 + q0w + j) * ld_row + hd * 64 + h2;
    const float f = MODE == 0 ? scale * LOG2E : 1.0f;
#pragma unroll
    for (int s = 0; s < 32; ++s) af[s] = ap[2 * s] * f;
  }
  const float* kbase = keyop + row0 * ld_key + hd * 64;
  float* obase = out + ((size_t)(b * heads + hd) * Tp) * Tp;
  const float* pbase = MODE == 1 ? Pin + ((size_t)(b * heads + hd) * Tp) * Tp : nullptr;
  const int ntiles = Tp / AR_K;
  const int key0 = tid >> 4, dq0 = tid & 15;  // staging: 32 keys x 64 d = 512 float4, two per thread (second: key0 + 16)
  float4 kr[2];
  auto fetch = [&](int kt) {
#pragma unroll
    for (int it = 0; it < 2; ++it)
      kr[it] = *reinterpret_cast<const float4*>(kbase + (size_t)(kt * AR_K + key0 + 16 * it) * ld_key + dq0 * 4);
  };
  auto park = [&](int buf) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      float* kd = Ks[buf] + (key0 + 16 * it) * AR_LD + dq0 * 4;
      kd[0] = kr[it].x; kd[1] = kr[it].y; kd[2] = kr[it].z; kd[3] = kr[it].w;
    }
  };
  if constexpr (MODE == 0) {
    // ---- sweep 1 (T-order): running max / sum per query, lane-local over its 16 keys of a tile
    float m_run = -1e30f, l_run = 0.f;
    fetch(0);
    park(0);
    __syncthreads();
    for (int kt = 0; kt < ntiles; ++kt) {
      const int cur = kt & 1;
      const bool more = kt + 1 < ntiles;
      if (more) fetch(kt + 1);
      const float* K = Ks[cur];
      floatx16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int t = 0; t < 32; ++t) s = __builtin_amdgcn_mfma_f32_32x32x2f32(K[j * AR_LD + 2 * t + h2], af[t], s, 0, 0, 0);
      float tmax = -1e30f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kt * AR_K + (r & 3) + 8 * (r >> 2) + 4 * h2;
        if (key >= T) s[r] = -1e30f;
        tmax = fmaxf(tmax, s[r]);
      }
      const float m_new = fmaxf(m_run, tmax);
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) psum += __builtin_amdgcn_exp2f(s[r] - m_new);
      l_run = l_run * __builtin_amdgcn_exp2f(m_run - m_new) + psum;
      m_run = m_new;
      if (more) park(cur ^ 1);
      __syncthreads();
    }
    {  // the two lanes of a query (h2 = 0 / 1) hold disjoint keys: merge, then (m, 1 / l) of the wave's 32 queries -> LDS
      const float m2 = __shfl_xor(m_run, 32, 64), l2 = __shfl_xor(l_run, 32, 64);
      const float mt = fmaxf(m_run, m2);
      const float lt = l_run * __builtin_amdgcn_exp2f(m_run - mt) + l2 * __builtin_amdgcn_exp2f(m2 - mt);
      if (h2 == 0) {
        stat[0][wave * 32 + j] = mt;
        stat[1][wave * 32 + j] = 1.0f / lt;
      }
    }
    __syncthreads();
  }
  // ---- the N-order sweep: lane = key column (lane & 31), rows kappa(r) + 4 h2 of the wave's 32 queries
  float rs0[16], rs1[16];  // per row: forward (m, 1 / l); backward (D, -)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qi = (r & 3) + 8 * (r >> 2) + 4 * h2;
    if constexpr (MODE == 0) {
      rs0[r] = stat[0][wave * 32 + qi];
      rs1[r] = q0w + qi < T ? stat[1][wave * 32 + qi] : 0.f;  // padded query rows: P = 0
    } else {
      rs0[r] = D[(size_t)(b * heads + hd) * Tp + q0w + qi];
      rs1[r] = scale;
    }
  }
  float pr[16];
  auto fetch_p = [&](int kt) {
    if constexpr (MODE == 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qi = (r & 3) + 8 * (r >> 2) + 4 * h2;
        pr[r] = pbase[(size_t)(q0w + qi) * Tp + kt * AR_K + j];
      }
    }
  };
  fetch(0);
  park(0);
  fetch_p(0);
  __syncthreads();
  for (int kt = 0; kt < ntiles; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < ntiles;
    if (more) fetch(kt + 1);
    const float* K = Ks[cur];
    floatx16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int t = 0; t < 32; ++t) s = __builtin_amdgcn_mfma_f32_32x32x2f32(af[t], K[j * AR_LD + 2 * t + h2], s, 0, 0, 0);
    const int key = kt * AR_K + j;
    float o[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if constexpr (MODE == 0) o[r] = key < T ? __builtin_amdgcn_exp2f(s[r] - rs0[r]) * rs1[r] : 0.f;
      else o[r] = rs1[r] * pr[r] * (s[r] - rs0[r]);
    }
    if (more) fetch_p(kt + 1);  // (behind the uses of this tile's P)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qi = (r & 3) + 8 * (r >> 2) + 4 * h2;
      obase[(size_t)(q0w + qi) * Tp + key] = o[r];
    }
    if (more) park(cur ^ 1);
    __syncthreads();
  }
}

// D[(b * heads + h) * Tp + t] = sum_d dO[b * Tp + t][64 h + d] * O[b * Tp + t][64 h + d] = rowsum(dP (.) P) of that (image, head, query)
// (O = P V, dP = dO V^T): what the softmax backward subtracts, from two [R][C] tensors instead of two [.., Tp][Tp] ones.  One
// wave per token row, 16 lanes per head pass (C / 64 heads, 4 per pass).
__global__ __launch_bounds__(256) void s2_rowdot_kernel(const float* __restrict__ dO, const float* __restrict__ O,
                                                        float* __restrict__ D, int R, int Tp, int C) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int b = r / Tp, t = r - b * Tp, heads = C >> 6;
  const float4* a = reinterpret_cast<const float4*>(dO + (size_t)r * C);
  const float4* o = reinterpret_cast<const float4*>(O + (size_t)r * C);
  for (int h0 = 0; h0 < heads; h0 += 4) {  // 64 lanes x float4 = 4 heads of 64 columns
    const int h = h0 + (lane >> 4);
    float v = h < heads ? f4_dot(a[h0 * 16 + lane], o[h0 * 16 + lane]) : 0.f;
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    if ((lane & 15) == 0 && h < heads) D[((size_t)b * heads + h) * Tp + t] = v;
  }
}

// ==========================================================================================================
// Loss and its gradient over rows n_prefix <= t < T of every image, one wave per row (main_denoiser.py:213-217;
// main_distillation.py: mse + 1 - cosine_similarity(dim=-1).mean()):
//   o = a + b with ADD (stage 2: the last residual add, n_prefix = 0), o = a without (stage 3: the final-normed x)
//   l2 = mean((o - t)^2) over the N C loss elements, N = batch * (T - n_prefix) rows
//   cos_t = o.t / (max(|o|, 1e-8) max(|t|, 1e-8)) (F.cosine_similarity, eps 1e-8);  loss = l2 + 1 - mean_t cos_t
//   dout = 2 (o - t) / (N C) - (t / (|o| |t|) - cos o / |o|^2) / N
// The two sums, of (o - t)^2 and of cos, are added over the workgroups' partials in acc as 128-bit fixed-point integers
// (loss_acc_add below): integer addition does not depend on the order in which the workgroups arrive, so the loss has the same
// bits on every run of the same input.  Prefix and padded rows: dout = 0.
// target and out (may be NULL; receives o) are packed [batch, T - n_prefix, C].
// ==========================================================================================================
// acc (64 floats, cleared by the caller, 8-byte aligned) as the loss kernels use it: sum i (0: squared error, 1: cosine) is the
// signed 128-bit integer (hi = u64[2 i + 1], lo = u64[2 i]) in units of 2^-64, floats [8 + i] take what that cannot hold.
// v, a workgroup's fp32 partial, is exact as a double; floor(v) and v - floor(v) are exact too, the fraction is cut below
// 2^-64 (a function of v alone).  lo is added with a returning 64-bit atomic and its carry goes into hi: both are additions
// modulo 2^64 of values that depend on v only, so the final 128 bits are the exact sum of the cut partials in any order.  A
// partial that is not finite, or at least 2^62 in size, goes to the float slot with a float atomic instead: the loss then
// comes out non-finite (or huge), which is what the trainers' non-finite check looks for.
__device__ __forceinline__ void loss_acc_add(float* acc, int i, float v) {
  if (!(fabsf(v) < 4.6e18f)) {  // (also NaN)
    atomic_add_f32(acc + 8 + i, v);
    return;
  }
  const double d = (double)v, fl = floor(d);
  const unsigned long long lo = (unsigned long long)((d - fl) * 18446744073709551616.0);  // < 2^64: the fraction is < 1
  unsigned long long hi = (unsigned long long)(long long)fl;
  unsigned long long* w = reinterpret_cast<unsigned long long*>(acc) + 2 * i;
  if (lo) {
    const unsigned long long old = __hip_atomic_fetch_add(w, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    hi += (old + lo < old) ? 1ull : 0ull;  // the carry out of the low word
  }
  if (hi) __hip_atomic_fetch_add(w + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the sum back as a float: one rounding to double of each word, one of their sum, one to float -- a function of the 128 bits
__device__ __forceinline__ float loss_acc_get(const float* acc, int i) {
  const unsigned long long* w = reinterpret_cast<const unsigned long long*>(acc) + 2 * i;
  const double v = (double)(long long)w[1] + (double)w[0] * (1.0 / 18446744073709551616.0);
  return (float)v + acc[8 + i];
}

template <int C, bool ADD>
__global__ __launch_bounds__(256) void s2_loss_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                      const float* __restrict__ target, float* __restrict__ out,
                                                      float* __restrict__ dout, float* __restrict__ acc, int n_prefix,
                                                      int T, int Tp, int R, float inv_el, float inv_tok) {
  __shared__ float part[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = blockIdx.x * 4 + wave;
  float se = 0.f, cs = 0.f;
  if (r < R) {
    const int img = r / Tp, t = r - img * Tp;
    Row<C> o;
    if (t < n_prefix || t >= T) {
      o.zero();
      o.store(dout + (size_t)r * C, lane);
    } else {
      const size_t pr = (size_t)img * (T - n_prefix) + (t - n_prefix);
      Row<C> y, tg;
      o.load(a + (size_t)r * C, lane);
      if (ADD) y.load(b + (size_t)r * C, lane);
      tg.load(target + pr * C, lane);
      float s_d = 0.f, s_ot = 0.f, s_oo = 0.f, s_tt = 0.f;
      ROW_FOR(j, Row<C>::NJ) {
        if (ADD) o.v[j] = f4_add(o.v[j], y.v[j]);
        const float4 d = f4_sub(o.v[j], tg.v[j]);
        s_d += f4_dot(d, d);
        s_ot += f4_dot(o.v[j], tg.v[j]);
        s_oo += f4_dot(o.v[j], o.v[j]);
        s_tt += f4_dot(tg.v[j], tg.v[j]);
      }
      if (out) o.store(out + pr * C, lane);
      s_d = wave_sum(s_d);
      s_ot = wave_sum(s_ot);
      s_oo = wave_sum(s_oo);
      s_tt = wave_sum(s_tt);
      const float no = fmaxf(sqrtf(s_oo), 1e-8f), nt = fmaxf(sqrtf(s_tt), 1e-8f);
      const float cosv = s_ot / (no * nt);
      const float ka = 2.0f * inv_el, kt = inv_tok / (no * nt), ko = inv_tok * cosv / (no * no);
      ROW_FOR(j, Row<C>::NJ) {
        const float4 d = f4_sub(o.v[j], tg.v[j]);
        float4 g;
        g.x = ka * d.x - (kt * tg.v[j].x - ko * o.v[j].x);
        g.y = ka * d.y - (kt * tg.v[j].y - ko * o.v[j].y);
        g.z = ka * d.z - (kt * tg.v[j].z - ko * o.v[j].z);
        g.w = ka * d.w - (kt * tg.v[j].w - ko * o.v[j].w);
        o.v[j] = g;
      }
      o.store(dout + (size_t)r * C, lane);
      se = s_d;
      cs = cosv;
    }
  }
  if (lane == 0) {
    part[0][wave] = se;
    part[1][wave] = cs;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    loss_acc_add(acc, 0, (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]));
    loss_acc_add(acc, 1, (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]));
  }
}

// loss_out = {l2 + 1 - cos, l2, 1 - cos, 0} from the two accumulated sums
__global__ void s2_loss_finish_kernel(const float* __restrict__ acc, float* __restrict__ out, float inv_el, float inv_tok) {
  const float l2 = loss_acc_get(acc, 0) * inv_el, cl = 1.0f - loss_acc_get(acc, 1) * inv_tok;
  out[0] = l2 + cl;
  out[1] = l2;
  out[2] = cl;
  out[3] = 0.f;
}

// out[k][n] = in[n][k] (n, k multiples of 32): 32 x 32 tiles through LDS, both sides in whole 128-B row pieces
__global__ __launch_bounds__(256) void s2_transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int n, int k) {
  __shared__ float tile[32][33];
  const int k0 = blockIdx.x * 32, n0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int i = 0; i < 4; ++i) tile[ty + 8 * i][tx] = in[(size_t)(n0 + ty + 8 * i) * k + k0 + tx];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) out[(size_t)(k0 + ty + 8 * i) * n + n0 + tx] = tile[tx][ty + 8 * i];
}

// gb[c] += db[c] for the q and v thirds of a qkv bias gradient [3 C]; the k third [C, 2 C) is left alone
__global__ __launch_bounds__(256) void s3_qv_bias_kernel(const float* __restrict__ db, float* __restrict__ gb, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < 3 * C && (c < C || c >= 2 * C)) gb[c] += db[c];
}

template <bool ADD>
int loss_rows_t(int C, const float* a, const float* b, const float* target, float* out, float* dout, float* acc, int n_prefix,
                int T, int Tp, int R, float inv_el, float inv_tok, hipStream_t s) {
  switch (C) {
    case 384: return launch_rows(s2_loss_kernel<384, ADD>, R, s, a, b, target, out, dout, acc, n_prefix, T, Tp, R, inv_el, inv_tok);
    case 768: return launch_rows(s2_loss_kernel<768, ADD>, R, s, a, b, target, out, dout, acc, n_prefix, T, Tp, R, inv_el, inv_tok);
    default: return launch_rows(s2_loss_kernel<1024, ADD>, R, s, a, b, target, out, dout, acc, n_prefix, T, Tp, R, inv_el, inv_tok);
  }
}

int attn_rows(int mode, const float* rowop, int ld_row, const float* keyop, int ld_key, const float* P, const float* D, float* out,
              int batch, int heads, int T, int Tp, float scale, hipStream_t s) {
  const dim3 grid((Tp / AR_Q) * heads * batch), blk(256);
  if (mode == 0)
    hipLaunchKernelGGL(s2_attn_rows_kernel<0>, grid, blk, 0, s, rowop, ld_row, keyop, ld_key, (const float*)nullptr,
                       (const float*)nullptr, out, heads, T, Tp, scale);
  else
    hipLaunchKernelGGL(s2_attn_rows_kernel<1>, grid, blk, 0, s, rowop, ld_row, keyop, ld_key, P, D, out, heads, T, Tp, scale);
  DVT_CHECK_LAUNCH();
  return 0;
}

int rowdot(const float* dO, const float* O, float* D, int R, int Tp, int C, hipStream_t s) {
  return launch_rows(s2_rowdot_kernel, R, s, dO, O, D, R, Tp, C);
}

// One of the six (image, head)-batched attention products
DvtGemmEx attn_gemm(const AttnDims& d, int layout, const float* A, int lda, long long sA0, long long sA1, const float* B,
                    int ldb, long long sB0, long long sB1, float* Cc, int ldc, long long sC0, long long sC1, int M, int N,
                    int K) {
  DvtGemmEx g{};
  g.layout = layout;
  g.A = A; g.B = B; g.C = Cc;
  g.M = M; g.N = N; g.K = K;
  g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.nb0 = d.batch; g.nb1 = d.heads;
  g.sA0 = sA0; g.sA1 = sA1; g.sB0 = sB0; g.sB1 = sB1; g.sC0 = sC0; g.sC1 = sC1;
  return g;
}

// batch strides (image, head) of the q / k / v columns of qkv, of P / dP, and of the per-head slices of an [R][C] tensor
struct AttnStrides {
  long long qs0, qs1, ps0, ps1, os0, os1;
  explicit AttnStrides(const AttnDims& d)
      : qs0((long long)d.Tp * 3 * d.C), qs1(64), ps0((long long)d.heads * d.Tp * d.Tp), ps1((long long)d.Tp * d.Tp),
        os0((long long)d.Tp * d.C), os1(64) {}
};

}  // namespace

struct SideStream {
  hipStream_t stream;
  hipEvent_t ev_fork, ev_join;
};

// the current device's side stream, or null: created whole or not at all (a later call tries again)
static const SideStream* side_stream() {
  static std::mutex lock;
  static std::map<int, SideStream> per_device;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> hold(lock);
  const auto it = per_device.find(dev);
  if (it != per_device.end()) return &it->second;
  SideStream n{};
  if (hipStreamCreateWithFlags(&n.stream, hipStreamNonBlocking) == hipSuccess &&
      hipEventCreateWithFlags(&n.ev_fork, hipEventDisableTiming) == hipSuccess &&
      hipEventCreateWithFlags(&n.ev_join, hipEventDisableTiming) == hipSuccess)
    return &per_device.emplace(dev, n).first->second;
  if (n.ev_fork) (void)hipEventDestroy(n.ev_fork);
  if (n.stream) (void)hipStreamDestroy(n.stream);
  return nullptr;
}

BlockFork::BlockFork(hipStream_t s, bool want) : s_(s), side_((want && g_s2_fork_wgrad) ? side_stream() : nullptr) {}

hipStream_t BlockFork::side() const { return side_ ? side_->stream : s_; }

int BlockFork::fork() {
  if (!side_) return 0;
  hipError_t e = hipEventRecord(side_->ev_fork, s_);
  if (e == hipSuccess) e = hipStreamWaitEvent(side_->stream, side_->ev_fork, 0);
  open_ = open_ || e == hipSuccess;
  return (int)e;
}

int BlockFork::join() {
  if (!open_) return 0;
  open_ = false;
  hipError_t e = hipEventRecord(side_->ev_join, side_->stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(s_, side_->ev_join, 0);
  return (int)e;
}

int loss_rows(bool add, int C, const float* a, const float* b, const float* target, float* out, float* dout, float* acc,
              int n_prefix, int T, int Tp, int R, int norm_batch, float* loss_out, hipStream_t s) {
  const float N = (float)norm_batch * (float)(T - n_prefix);
  const float inv_el = 1.0f / (N * C), inv_tok = 1.0f / N;
  const hipError_t e = hipMemsetAsync(acc, 0, 64 * sizeof(float), s);
  if (e != hipSuccess) return (int)e;
  if (add) DVT_TRY(loss_rows_t<true>(C, a, b, target, out, dout, acc, n_prefix, T, Tp, R, inv_el, inv_tok, s));
  else DVT_TRY(loss_rows_t<false>(C, a, b, target, out, dout, acc, n_prefix, T, Tp, R, inv_el, inv_tok, s));
  hipLaunchKernelGGL(s2_loss_finish_kernel, dim3(1), dim3(1), 0, s, (const float*)acc, loss_out, inv_el, inv_tok);
  DVT_CHECK_LAUNCH();
  return 0;
}

int ln_bwd(int C, const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
           const float* dres, float* dx, float* dgamma, float* dbeta, int R, hipStream_t s) {
  const dim3 grid(dvt_cdiv(R, 32)), blk(256);
  switch (C) {
    case 384: hipLaunchKernelGGL(s2_ln_bwd_kernel<384>, grid, blk, 0, s, dy, x, mean, rstd, gamma, dres, dx, dgamma, dbeta, R); break;
    case 768: hipLaunchKernelGGL(s2_ln_bwd_kernel<768>, grid, blk, 0, s, dy, x, mean, rstd, gamma, dres, dx, dgamma, dbeta, R); break;
    default: hipLaunchKernelGGL(s2_ln_bwd_kernel<1024>, grid, blk, 0, s, dy, x, mean, rstd, gamma, dres, dx, dgamma, dbeta, R); break;
  }
  DVT_CHECK_LAUNCH();
  return 0;
}

int gelu_fwd(const float* h, float* a, int64_t n4, hipStream_t s) {
  hipLaunchKernelGGL(s2_gelu_kernel, dim3(dvt_cdiv(n4, 256)), dim3(256), 0, s, (const float4*)h, (float4*)a, n4);
  DVT_CHECK_LAUNCH();
  return 0;
}

int gelu_bwd(const float* h, float* da, int64_t n4, hipStream_t s) {
  hipLaunchKernelGGL(s2_gelu_bwd_kernel, dim3(dvt_cdiv(n4, 256)), dim3(256), 0, s, (const float4*)h, (float4*)da, n4);
  DVT_CHECK_LAUNCH();
  return 0;
}

int lin_fwd(const float* x, const float* w, const float* b, float* y, int R, int n, int k, hipStream_t s) {
  // round 6: the forward linear layers take the fp32 extractor's 128 x 128 x 32 tile where the shape allows (R = batch x 1408
  // rows, n and k multiples of 128 / 32: every layer of the Block) -- 125 against 97 TF/s; summation order differs only
  if (g_s2_big_fwd && dvt_linear_big_ok(R, n, k)) return dvt_linear_fwd_big(x, w, b, y, R, n, k, s);
  DvtGemmEx g{};
  g.layout = 0;
  g.A = x; g.B = w; g.C = y;
  g.M = R; g.N = n; g.K = k;
  g.lda = k; g.ldb = k; g.ldc = n;
  g.bias = b;
  return dvt_gemm_f32_ex(&g, s);
}

// wT (round 6): scratch for w^T [k][n].  With it the data gradient is a FORWARD linear layer of the transposed weight --
// dx = dy . (w^T)^T -- and takes the 128 x 128 x 32 tile (dvt_linear_fwd_big: both operands k-contiguous); the transposition is
// 2 x 9 MB of traffic at most per layer, the GEMM 0.07-0.2 TFLOP.  Summation order differs from the 64 x 64 kernel only.
int lin_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* db, int R, int n, int k,
            hipStream_t s, float* wT) {
  // Round 6: the weight gradient and the data gradient of a layer are independent products of the same dy.  Their grids are a few
  // rounds of the chip's 512 workgroup slots each (2112 tiles = 4.1 rounds for the 768-wide outputs: the last round is 1/8
  // full), so the weight gradient goes to a side stream and the two fill each other's tails; joined before this returns (the
  // caller's next kernels overwrite dy / x).
  BlockFork f(s, dx != nullptr);
  DVT_TRY(f.fork());
  const hipStream_t sw = f.side();
  if (g_s2_big_wgrad && dvt_linear_wgrad_big_ok(R, n, k)) {  // round 6: the weight gradient on the 128 x 128 tile too
    DVT_TRY(dvt_linear_wgrad_big(dy, x, dw, db, R, n, k, 1, sw));
  } else {
    DvtGemmEx g{};
    g.layout = 2;
    g.A = dy; g.B = x; g.C = dw;
    g.M = n; g.N = k; g.K = R;
    g.lda = n; g.ldb = k; g.ldc = k;
    g.colsum = db;
    g.accumulate = 1;
    DVT_TRY(dvt_gemm_f32_ex(&g, sw));
  }
  if (!dx) return 0;
  if (wT && g_s2_big_bwd && n % 32 == 0 && k % 32 == 0 && dvt_linear_big_ok(R, k, n)) {
    hipLaunchKernelGGL(s2_transpose_kernel, dim3(k / 32, n / 32), dim3(256), 0, s, w, wT, n, k);
    DVT_CHECK_LAUNCH();
    DVT_TRY(dvt_linear_fwd_big(dy, wT, nullptr, dx, R, k, n, s));
  } else {
    DvtGemmEx d{};
    d.layout = 1;
    d.A = dy; d.B = w; d.C = dx;
    d.M = R; d.N = k; d.K = n;
    d.lda = n; d.ldb = k; d.ldc = k;
    DVT_TRY(dvt_gemm_f32_ex(&d, s));
  }
  return f.join();
}

int block_attn_fwd(const AttnDims& d, const float* qkv, float* P, float* ao, float scale, bool rows_kernel, hipStream_t s) {
  const int C = d.C, Tp = d.Tp;
  const AttnStrides st(d);
  DvtGemmEx g{};
  if (rows_kernel) {  // round 6: q k^T and the softmax in one kernel, P written once
    DVT_TRY(attn_rows(0, qkv, 3 * C, qkv + C, 3 * C, nullptr, nullptr, P, d.batch, d.heads, d.T, Tp, scale, s));
  } else {
    g = attn_gemm(d, 0, qkv, 3 * C, st.qs0, st.qs1, qkv + C, 3 * C, st.qs0, st.qs1, P, Tp, st.ps0, st.ps1, Tp, Tp, 64);
    DVT_TRY(dvt_gemm_f32_ex(&g, s));
    DVT_TRY(s2_softmax(P, d.T, Tp, (int64_t)d.batch * d.heads * Tp, scale, s));
  }
  g = attn_gemm(d, 1, P, Tp, st.ps0, st.ps1, qkv + 2 * C, 3 * C, st.qs0, st.qs1, ao, C, st.os0, st.os1, Tp, 64, Tp);
  return dvt_gemm_f32_ex(&g, s);
}

int block_attn_bwd(const AttnDims& d, const float* qkv, const float* P, const float* ao, const float* dao, float* dqkv,
                   float* dP, float* rowdot_buf, float scale, bool rows_kernel, bool fuse_softmax_bwd, hipStream_t s) {
  const int C = d.C, Tp = d.Tp, R = d.batch * Tp;
  const AttnStrides st(d);
  // dV = P^T dao -- independent of the dS chain below (both read P and dao): on the side stream beside it (round 6, as the weight
  // gradients in lin_bwd); dq and dk, two products of the same dS, likewise.  Joined before the caller's lin_bwd reads dqkv.
  BlockFork f(s);
  const hipStream_t sv = f.side();
  DVT_TRY(f.fork());
  DvtGemmEx g = attn_gemm(d, 2, P, Tp, st.ps0, st.ps1, dao, C, st.os0, st.os1, dqkv + 2 * C, 3 * C, st.qs0, st.qs1, Tp, 64, Tp);
  DVT_TRY(dvt_gemm_f32_ex(&g, sv));
  // dP = dao v^T, and the softmax backward dS = scale P (.) (dP - rowsum(dP (.) P)).  Round 6: rowsum(dP (.) P) = dao . ao per
  // (image, head, query) comes from the two [R][C] tensors (s2_rowdot_kernel) and the backward is the EPILOGUE of the dP
  // product -- dP is never written, P read once (before: 3 GB written + 9 GB read + 3 GB written by s2_softmax_bwd_kernel)
  g = attn_gemm(d, 0, dao, C, st.os0, st.os1, qkv + 2 * C, 3 * C, st.qs0, st.qs1, dP, Tp, st.ps0, st.ps1, Tp, Tp, 64);
  if (fuse_softmax_bwd && rows_kernel) {
    DVT_TRY(rowdot(dao, ao, rowdot_buf, R, Tp, C, s));
    DVT_TRY(attn_rows(1, dao, C, qkv + 2 * C, 3 * C, P, rowdot_buf, dP, d.batch, d.heads, d.T, Tp, scale, s));
  } else if (fuse_softmax_bwd) {
    DVT_TRY(rowdot(dao, ao, rowdot_buf, R, Tp, C, s));
    g.smul = P;
    g.rowsub = rowdot_buf;
    g.oscale = scale;
    DVT_TRY(dvt_gemm_f32_ex(&g, s));
  } else {
    DVT_TRY(dvt_gemm_f32_ex(&g, s));
    DVT_TRY(s2_softmax_bwd(P, dP, Tp, (int64_t)d.batch * d.heads * Tp, scale, s));
  }
  // dq = dS k (main stream),  dk = dS^T q (side stream: behind dV there, and behind dS here)
  DVT_TRY(f.fork());
  g = attn_gemm(d, 1, dP, Tp, st.ps0, st.ps1, qkv + C, 3 * C, st.qs0, st.qs1, dqkv, 3 * C, st.qs0, st.qs1, Tp, 64, Tp);
  DVT_TRY(dvt_gemm_f32_ex(&g, s));
  g = attn_gemm(d, 2, dP, Tp, st.ps0, st.ps1, qkv, 3 * C, st.qs0, st.qs1, dqkv + C, 3 * C, st.qs0, st.qs1, Tp, 64, Tp);
  DVT_TRY(dvt_gemm_f32_ex(&g, sv));
  return f.join();
}

int add_ln(int C, const float* a, int a_packed, const float* b, int b_is_pos, float* sum_out, const float* g,
           const float* be, float* xn, float* mean, float* rstd, int T, int Tp, int R, float eps, hipStream_t s) {
  switch (C) {
    case 384: return launch_rows(s2_add_ln_kernel<384>, R, s, a, a_packed, b, b_is_pos, sum_out, g, be, xn, mean, rstd, T, Tp, R, eps);
    case 768: return launch_rows(s2_add_ln_kernel<768>, R, s, a, a_packed, b, b_is_pos, sum_out, g, be, xn, mean, rstd, T, Tp, R, eps);
    default: return launch_rows(s2_add_ln_kernel<1024>, R, s, a, a_packed, b, b_is_pos, sum_out, g, be, xn, mean, rstd, T, Tp, R, eps);
  }
}

int ls_add_ln(int C, const float* a, const float* f, const float* ls, float* sum_out, const float* g, const float* be,
              float* xn, float* mean, float* rstd, int T, int Tp, int R, float eps, hipStream_t s) {
  switch (C) {
    case 384: return launch_rows(s3_ls_add_ln_kernel<384>, R, s, a, f, ls, sum_out, g, be, xn, mean, rstd, T, Tp, R, eps);
    case 768: return launch_rows(s3_ls_add_ln_kernel<768>, R, s, a, f, ls, sum_out, g, be, xn, mean, rstd, T, Tp, R, eps);
    default: return launch_rows(s3_ls_add_ln_kernel<1024>, R, s, a, f, ls, sum_out, g, be, xn, mean, rstd, T, Tp, R, eps);
  }
}

static int ls_bwd(int C, const float* dy, const float* f, const float* ls, float* df, float* dls, int R, hipStream_t s) {
  const dim3 grid(dvt_cdiv(R, 32)), blk(256);
  switch (C) {
    case 384: hipLaunchKernelGGL(s3_ls_bwd_kernel<384>, grid, blk, 0, s, dy, f, ls, df, dls, R); break;
    case 768: hipLaunchKernelGGL(s3_ls_bwd_kernel<768>, grid, blk, 0, s, dy, f, ls, df, dls, R); break;
    default: hipLaunchKernelGGL(s3_ls_bwd_kernel<1024>, grid, blk, 0, s, dy, f, ls, df, dls, R); break;
  }
  DVT_CHECK_LAUNCH();
  return 0;
}

// ---- a linear layer of the block, exact fp32 (mp null) or, stage 3's gemm_mode 1, its forward and data gradient on the
// extractor's bf16 GEMM (dvt_vit_gemm.hip, EPI_F32: bf16 operands, fp32 accumulation, fp32 output; m % 128 == n % 128 ==
// k % 64 == 0, which stage 3's check_cfg guarantees for every layer of the block: R = batch s_pad with s_pad % 128 == 0, dim in
// {384, 768, 1024}, mlp_dim % 128 == 0).  The A operand is rounded into `abf` right here; the weights (j: qkv, proj, fc1, fc2)
// were rounded by the caller. ----
static bool mp_shape_ok(int R, int n, int k) { return R > 0 && R % 128 == 0 && n % 128 == 0 && k % 64 == 0; }

// y[R][n] = x[R][k] . w[n][k]^T + b
static int blk_lin_fwd(const BlockBf16* mp, int j, const float* x, const float* w, const float* b, float* y, int R, int n, int k,
                       hipStream_t s) {
  if (!mp) return lin_fwd(x, w, b, y, R, n, k, s);
  if (!mp_shape_ok(R, n, k)) return DVT_E_BADARG;
  DVT_TRY(dvt_s3_cast_bf16(x, mp->abf, R, k, s));
  return dvt_vit_gemm_f32out(mp->abf, mp->w[j], b, y, R, n, k, s);
}

// dx[R][k] = dy[R][n] . w[n][k];  dw[n][k] += dy^T . x and db[n] += colsum(dy), with mp too in exact fp32 from the UNROUNDED dy
// and x, on lin_bwd's side stream beside the data gradient as in the fp32 mode -- or, with mp->xbf, dw from the rounded operands
static int blk_lin_bwd(const BlockBf16* mp, int j, const float* dy, const float* x, const float* w, float* dx, float* dw, float* db,
                       int R, int n, int k, hipStream_t s, float* wT) {
  if (!mp) return lin_bwd(dy, x, w, dx, dw, db, R, n, k, s, wT);
  if (!mp_shape_ok(R, k, n)) return DVT_E_BADARG;
  BlockFork f(s);
  if (mp->xbf) {  // gemm_modes 5 / 7: dw from the rounded dy and x.  The side stream starts behind dy's cast, which both products read
    if (k % 128) return DVT_E_BADARG;
    DVT_TRY(dvt_s3_cast_bf16(dy, mp->abf, R, n, s));
    DVT_TRY(f.fork());
    DVT_TRY(dvt_s3_cast_bf16(x, mp->xbf, R, k, f.side()));
    DVT_TRY(dvt_s3_wgrad_bf16_run(mp->abf, mp->xbf, dy, dw, db, mp->wpart, R, n, k, dvt_s3_wgrad_splits(R, n, k), 1, f.side()));
    DVT_TRY(dvt_vit_gemm_f32out(mp->abf, mp->wt[j], nullptr, dx, R, k, n, s));
    return f.join();
  }
  DVT_TRY(f.fork());
  DVT_TRY(lin_bwd(dy, x, nullptr, nullptr, dw, db, R, n, k, f.side()));  // no dx: the weight and bias gradients alone, beside
  DVT_TRY(dvt_s3_cast_bf16(dy, mp->abf, R, n, s));
  DVT_TRY(dvt_vit_gemm_f32out(mp->abf, mp->wt[j], nullptr, dx, R, k, n, s));
  return f.join();
}

// ---- the block (dvt_block_train.h): x1 = xin + [ls1 (.)] proj(attn(norm1 xin)), out = x1 + [ls2 (.)] fc2(gelu(fc1(norm2 x1))) ----
static const float kAttnScale = 0.125f;  // head_dim^-0.5
enum { WQKV = 0, WPROJ, WFC1, WFC2 };

int block_fwd(const BlockDims& d, const BlockTensors<const float>& p, const BlockActs& k, const BlockBf16* mp, bool rows_kernel,
              hipStream_t s) {
  const int C = d.ad.C, F = d.F, T = d.ad.T, Tp = d.ad.Tp, R = d.ad.batch * Tp;
  DVT_TRY(blk_lin_fwd(mp, WQKV, k.xn1, p.qkvw, p.qkvb, k.qkv, R, 3 * C, C, s));
  if (mp && mp->aq)  // gemm_mode 3: ao and lse, no P
    DVT_TRY(dvt_s3_attn_fwd(k.qkv, mp->aq, k.ao, mp->lse, d.ad.batch, d.ad.heads, T, Tp, s));
  else
    DVT_TRY(block_attn_fwd(d.ad, k.qkv, k.P, k.ao, kAttnScale, rows_kernel, s));  // P = softmax(scale q k^T), ao = P v
  DVT_TRY(blk_lin_fwd(mp, WPROJ, k.ao, p.projw, p.projb, k.f1, R, C, C, s));
  DVT_TRY(resid_ln(C, k.xin, k.f1, p.ls1, k.x1, p.n2w, p.n2b, k.xn2, k.mean2, k.rstd2, T, Tp, R, d.eps, s));
  DVT_TRY(blk_lin_fwd(mp, WFC1, k.xn2, p.fc1w, p.fc1b, k.h, R, F, C, s));
  DVT_TRY(gelu_fwd(k.h, k.a, (int64_t)R * F / 4, s));
  return blk_lin_fwd(mp, WFC2, k.a, p.fc2w, p.fc2b, k.f2, R, C, F, s);
}

int block_bwd(const BlockDims& d, const BlockTensors<const float>& p, const BlockTensors<float>& g, const BlockActs& k,
              const BlockScratch& w, const BlockBf16* mp, bool rows_kernel, bool fuse_softmax_bwd, hipStream_t s) {
  const int C = d.ad.C, F = d.F, R = d.ad.batch * d.ad.Tp;
  // mlp: out = x1 + [ls2 (.)] f2
  const float* dy = w.d0;
  if (p.ls2) {
    DVT_TRY(ls_bwd(C, w.d0, k.f2, p.ls2, w.d1, g.ls2, R, s));  // d1 = d f2
    dy = w.d1;
  }
  DVT_TRY(blk_lin_bwd(mp, WFC2, dy, k.a, p.fc2w, w.dh, g.fc2w, g.fc2b, R, C, F, s, w.wT));
  DVT_TRY(gelu_bwd(k.h, w.dh, (int64_t)R * F / 4, s));
  DVT_TRY(blk_lin_bwd(mp, WFC1, w.dh, k.xn2, p.fc1w, w.d2, g.fc1w, g.fc1b, R, F, C, s, w.wT));
  DVT_TRY(ln_bwd(C, w.d2, k.x1, k.mean2, k.rstd2, p.n2w, w.d0, w.d1, g.n2w, g.n2b, R, s));  // d1 = d x1
  // attention: x1 = xin + [ls1 (.)] f1
  dy = w.d1;
  if (p.ls1) {
    DVT_TRY(ls_bwd(C, w.d1, k.f1, p.ls1, w.d0, g.ls1, R, s));  // d0 = d f1
    dy = w.d0;
  }
  DVT_TRY(blk_lin_bwd(mp, WPROJ, dy, k.ao, p.projw, w.d2, g.projw, g.projb, R, C, C, s, w.wT));  // d2 = d ao
  if (mp && mp->aq)
    DVT_TRY(dvt_s3_attn_bwd(mp->aq, k.ao, w.d2, mp->lse, w.rowdot, w.dqkv, d.ad.batch, d.ad.heads, d.ad.T, d.ad.Tp, s));
  else
    DVT_TRY(block_attn_bwd(d.ad, k.qkv, k.P, k.ao, w.d2, w.dqkv, w.dP, w.rowdot, kAttnScale, rows_kernel, fuse_softmax_bwd, s));
  if (mp && mp->aq) {  // the bias gradient without its k third, which is identically zero (BlockBf16)
    const hipError_t e = hipMemsetAsync(mp->qkv_db, 0, sizeof(float) * 3 * C, s);
    if (e != hipSuccess) return (int)e;
    DVT_TRY(blk_lin_bwd(mp, WQKV, w.dqkv, k.xn1, p.qkvw, w.d2, g.qkvw, mp->qkv_db, R, 3 * C, C, s, w.wT));
    hipLaunchKernelGGL(s3_qv_bias_kernel, dim3(dvt_cdiv(3 * C, 256)), dim3(256), 0, s, (const float*)mp->qkv_db, g.qkvb, C);
    DVT_CHECK_LAUNCH();
  } else {
    DVT_TRY(blk_lin_bwd(mp, WQKV, w.dqkv, k.xn1, p.qkvw, w.d2, g.qkvw, g.qkvb, R, 3 * C, C, s, w.wT));
  }
  return ln_bwd(C, w.d2, k.xin, k.mean1, k.rstd1, p.n1w, w.d1, w.d0, g.n1w, g.n1b, R, s);  // d0 = d xin
}

void carve_block_acts(Carver& cv, BlockActs* k, int64_t R, int64_t C, int64_t F, int64_t PP, bool own_f, bool own_qkv) {
  k->xin = cv.take(R * C);
  k->xn1 = cv.take(R * C);
  k->mean1 = cv.take(R);
  k->rstd1 = cv.take(R);
  k->qkv = own_qkv ? cv.take(R * 3 * C) : nullptr;
  k->P = cv.take(PP);
  k->ao = cv.take(R * C);
  k->f1 = own_f ? cv.take(R * C) : nullptr;
  k->x1 = cv.take(R * C);
  k->xn2 = cv.take(R * C);
  k->mean2 = cv.take(R);
  k->rstd2 = cv.take(R);
  k->h = cv.take(R * F);
  k->a = cv.take(R * F);
  k->f2 = own_f ? cv.take(R * C) : nullptr;
}

void carve_block_scratch(Carver& cv, BlockScratch* w, int64_t R, int64_t C, int64_t F, int64_t PP, int64_t rowdot_floats) {
  w->d0 = cv.take(R * C);
  w->d1 = cv.take(R * C);
  w->d2 = cv.take(R * C);
  w->dh = cv.take(R * F);
  w->dqkv = cv.take(R * 3 * C);
  w->dP = cv.take(PP);
  w->acc = cv.take(64);
  w->wT = cv.take((3 * C > F ? 3 * C : F) * C);  // one transposed weight matrix, rebuilt in front of each data-gradient GEMM
  w->rowdot = cv.take(rowdot_floats);            // [batch * heads * Tp] rowsum(dP (.) P) of the softmax backward
}

void carve_block_bf16(Carver& cv, BlockBf16* bf, int nb, int64_t R, int64_t C, int64_t F, int64_t lse_floats, int mode) {
  if (!(mode & MODE_GEMM)) return;
  auto take16 = [&](int64_t halves) { return reinterpret_cast<uint16_t*>(cv.take((halves + 1) / 2)); };
  const int64_t wn[4] = {3 * C * C, C * C, F * C, C * F};
  for (int b = 0; b < nb; ++b)
    for (int i = 0; i < 4; ++i) {
      bf[b].w[i] = take16(wn[i]);
      bf[b].wt[i] = take16(wn[i]);
    }
  uint16_t* abf = take16(R * (3 * C > F ? 3 * C : F));  // the widest A operand: a / dh [R, mlp_dim] or dqkv [R, 3 dim]
  for (int b = 0; b < nb; ++b) bf[b].abf = abf;
  if (mode & MODE_ATTN) {
    for (int b = 0; b < nb; ++b) {
      bf[b].aq = take16(3 * R * C);
      bf[b].lse = cv.take(lse_floats);
    }
    float* qkv_db = cv.take(3 * C);
    for (int b = 0; b < nb; ++b) bf[b].qkv_db = qkv_db;
  }
  if (mode & MODE_WGRAD) {  // behind modes 1 and 3: the widest layer input's row cast, and the largest layer's partial tiles
    uint16_t* xbf = take16(R * (F > C ? F : C));
    const int ln[4] = {(int)(3 * C), (int)C, (int)F, (int)C}, lk[4] = {(int)C, (int)C, (int)C, (int)F};
    int64_t part = 0;
    for (int i = 0; i < 4; ++i) {
      const int64_t p = dvt_s3_wgrad_partial_bytes(R, ln[i], lk[i], dvt_s3_wgrad_splits(R, ln[i], lk[i]));
      part = p > part ? p : part;
    }
    void* wpart = cv.take(part / 4);
    for (int b = 0; b < nb; ++b) bf[b].xbf = xbf, bf[b].wpart = wpart;
  }
}

int cast_block_weights(const BlockTensors<const float>& p, const BlockBf16& bf, int C, int F, hipStream_t s) {
  const int wn[4] = {3 * C, C, F, C}, wk[4] = {C, C, C, F};
  const float* wf[4] = {p.qkvw, p.projw, p.fc1w, p.fc2w};
  for (int j = 0; j < 4; ++j) {
    DVT_TRY(dvt_s3_cast_bf16(wf[j], bf.w[j], wn[j], wk[j], s));
    DVT_TRY(dvt_s3_cast_bf16_t(wf[j], bf.wt[j], wn[j], wk[j], s));
  }
  return 0;
}

// ---- component entry points for tests (include/dvt_parts.h): forwarders to the launchers above; no kernel and no launch of
// their own, every check in front of the first launch ----
extern "C" int dvt_parts_lin_fwd(const float* x, const float* w, const float* b, float* y, int R, int n, int k, void* stream) {
  s2_read_env();
  if (!x || !w || !y || R <= 0 || n <= 0 || k <= 0 || (n & 3) || (k & 3)) return DVT_E_BADARG;
  if (!(g_s2_big_fwd && dvt_linear_big_ok(R, n, k)) && (k % 64)) return DVT_E_BADARG;  // dvt_gemm_f32_ex: whole k-tiles
  return lin_fwd(x, w, b, y, R, n, k, (hipStream_t)stream);
}

extern "C" int dvt_parts_lin_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* db, float* wT,
                                 int R, int n, int k, void* stream) {
  s2_read_env();
  if (!dy || !x || !dw || !db || (dx && !w) || R <= 0 || n <= 0 || k <= 0) return DVT_E_BADARG;
  if ((n % 64) || (k % 64) || (R % 32)) return DVT_E_BADARG;
  // the 64 x 64 weight-gradient kernel reduces over whole 64-row tiles, and so does the layout-1 data gradient's operand
  if ((R % 64) && !(g_s2_big_wgrad && dvt_linear_wgrad_big_ok(R, n, k))) return DVT_E_BADARG;
  return lin_bwd(dy, x, w, dx, dw, db, R, n, k, (hipStream_t)stream, wT);
}

extern "C" int dvt_parts_attn_rows(int mode, const float* rowop, int ld_row, const float* keyop, int ld_key, const float* P,
                                   const float* D, float* out, int batch, int heads, int T, int Tp, float scale, void* stream) {
  if ((mode != 0 && mode != 1) || !rowop || !keyop || !out || batch < 1 || heads < 1 || Tp < AR_Q || (Tp % AR_Q) || T < 1 || T > Tp)
    return DVT_E_BADARG;
  if (ld_row < heads * 64 || ld_key < heads * 64 || (ld_key & 3) || !dvt_aligned16(keyop) || (mode == 1 && (!P || !D)))
    return DVT_E_BADARG;
  if ((int64_t)(Tp / AR_Q) * heads * batch > 0x7fffffffLL) return DVT_E_BADARG;
  return attn_rows(mode, rowop, ld_row, keyop, ld_key, P, D, out, batch, heads, T, Tp, scale, (hipStream_t)stream);
}

extern "C" int dvt_parts_rowdot(const float* dO, const float* O, float* D, int R, int Tp, int C, void* stream) {
  if (!dO || !O || !D || R < 1 || Tp < 1 || (R % Tp) || C < 64 || (C % 64) || !dvt_aligned16(dO) || !dvt_aligned16(O)) return DVT_E_BADARG;
  return rowdot(dO, O, D, R, Tp, C, (hipStream_t)stream);
}

extern "C" int dvt_parts_ln_bwd(int C, const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                                const float* dres, float* dx, float* dgamma, float* dbeta, int R, void* stream) {
  if (!parts_c_ok(C) || !dy || !x || !mean || !rstd || !gamma || !dx || !dgamma || !dbeta || R < 1) return DVT_E_BADARG;
  return ln_bwd(C, dy, x, mean, rstd, gamma, dres, dx, dgamma, dbeta, R, (hipStream_t)stream);
}

extern "C" int dvt_parts_gelu(const float* h, float* a, int64_t n4, int backward, void* stream) {
  if (!h || !a || n4 < 1 || !dvt_aligned16(h) || !dvt_aligned16(a) || (backward != 0 && backward != 1)) return DVT_E_BADARG;
  return backward ? gelu_bwd(h, a, n4, (hipStream_t)stream) : gelu_fwd(h, a, n4, (hipStream_t)stream);
}

extern "C" int dvt_parts_loss_rows(int C, const float* a, const float* b, const float* target, float* out, float* dout, float* acc,
                                   int n_prefix, int T, int Tp, int R, int norm_batch, float* loss_out, int add, void* stream) {
  if (!parts_c_ok(C) || !a || !target || !dout || !acc || !loss_out || (add && !b) || (add != 0 && add != 1)) return DVT_E_BADARG;
  if (reinterpret_cast<uintptr_t>(acc) & 7) return DVT_E_BADARG;  // (the loss sums are 64-bit words)
  if (n_prefix < 0 || T <= n_prefix || Tp < T || R < 1 || (R % Tp) || norm_batch < R / Tp) return DVT_E_BADARG;
  return loss_rows(add != 0, C, a, add ? b : nullptr, target, out, dout, acc, n_prefix, T, Tp, R, norm_batch, loss_out,
                   (hipStream_t)stream);
}

extern "C" int dvt_parts_add_ln(int C, const float* a, int a_packed, const float* b, int b_is_pos, float* sum_out,
                                const float* gamma, const float* beta, float* xn, float* mean, float* rstd, int T, int Tp, int R,
                                float eps, void* stream) {
  if (!parts_c_ok(C) || !a || !gamma || !beta || !xn || !mean || !rstd || T < 1 || Tp < T || R < 1 || (R % Tp) || !(eps > 0.f))
    return DVT_E_BADARG;
  return add_ln(C, a, a_packed, b, b_is_pos, sum_out, gamma, beta, xn, mean, rstd, T, Tp, R, eps, (hipStream_t)stream);
}

extern "C" int dvt_parts_ls_add_ln(int C, const float* a, const float* f, const float* ls, float* sum_out, const float* gamma,
                                   const float* beta, float* xn, float* mean, float* rstd, int T, int Tp, int R, float eps,
                                   void* stream) {
  if (!parts_c_ok(C) || !a || (ls && !f) || !gamma || !beta || !xn || !mean || !rstd || T < 1 || Tp < T || R < 1 || (R % Tp) ||
      !(eps > 0.f))
    return DVT_E_BADARG;
  return ls_add_ln(C, a, f, ls, sum_out, gamma, beta, xn, mean, rstd, T, Tp, R, eps, (hipStream_t)stream);
}

extern "C" int dvt_parts_ls_bwd(int C, const float* dy, const float* f, const float* ls, float* df, float* dls, int R, void* stream) {
  if (!parts_c_ok(C) || !dy || !f || !ls || !df || !dls || R < 1) return DVT_E_BADARG;
  return ls_bwd(C, dy, f, ls, df, dls, R, (hipStream_t)stream);
}
