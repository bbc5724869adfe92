// bf16 flash attention of the stage-3 step's gemm_mode 3 (include/dvt_stage3.h): a forward that keeps one fp32 number per
// query row -- lse = log2 sum_k 2^(q' . k), q' = q log2(e) / 8 -- instead of the [Tp][Tp] probabilities, and a backward that
// recomputes P = 2^(q' . k - lse) tile by tile.  Head dimension 64, Tp % 128 == 0, keys and queries >= T masked.
//
// Operands: s3_attn_prep_kernel rounds q' , k and v ONCE to bf16 (round to nearest even) into [3][batch * heads][Tp][64]; d ao is
// rounded where a tile of it is staged; P and dS are rounded where they become MFMA operands.  Everything accumulated (the
// products, the running max / sum, lse, D = d ao . ao) is fp32.
//
// Every kernel: one workgroup = 128 rows of one (image, head), 4 waves x 32 rows whose operands stay in registers, sweeping the
// other side in 32-row tiles through LDS (two buffers, one barrier per tile).  v_mfma_f32_32x32x16_bf16 throughout, always in
// the orientation whose 32 x 32 result has the SWEPT index in its 16 registers and the wave's own row on the lane:
//   * what a row needs once per tile (running max / sum, lse, D, the mask of its own index) is lane-local;
//   * the result, packed to bf16, IS the B operand of the product that sums over the swept index -- registers 8 s .. 8 s + 7 are
//     swept rows 16 s + 8 (j >> 2) + 4 (lane >> 5) + (j & 3), so the A operand of that product takes its 8 elements from the
//     same rows: two 8-byte reads of the TRANSPOSED tile [d][32 swept rows] that the staging threads write beside the
//     row-major one.
//   forward   S^T = K Q'^T,  O^T += V^T P^T                                         (2 products)
//   dq        S^T = K Q'^T,  dP^T = V dO^T,  dQ^T += K^T dS^T                       (3 products)
//   dk, dv    S = Q' K^T,  dP = dO V^T,  dV^T += dO^T P,  dK^T += Q'^T dS           (4 products)
// dS = P (.) (dP - D) is the gradient of the natural-log logit q . k / 8: dq = dS k / 8, dk = dS^T q / 8 = ln 2 dS^T q'.
// No atomics and no reduction across workgroups: dq is owned by its query block, dk / dv by their key block, each recomputes S
// (9 tile products instead of 7), and two runs give the same bits.
//
// LDS images: row-major tiles with a pitch of 72 bf16 (144 B: the 16-byte fragment reads of 8 consecutive rows start in 8
// different 16-byte columns of the 128-byte bank row), transposed tiles with a pitch of 36 bf16 (72 B).
#include "dvt_vit_dev.h"
#include "../../include/dvt_parts.h"
#include "../../include/dvt_stage3.h"

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int SA_Q = 128;  // rows of a workgroup
constexpr int SA_T = 32;   // rows of a swept tile
constexpr int SA_RP = 72;  // pitch of a row-major tile [32][64], bf16
constexpr int SA_TP = 36;  // pitch of a transposed tile [64][32], bf16
constexpr int SA_ROW = SA_T * SA_RP, SA_TR = 64 * SA_TP;
constexpr float SA_LOG2E = 1.4426950408889634f, SA_LN2 = 0.6931471805599453f;
constexpr float SA_QSCALE = 0.125f * SA_LOG2E;  // head_dim^-0.5 log2(e)
constexpr float SA_NEG = -1e30f;

__device__ __forceinline__ floatx16 zero16() {
  floatx16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// registers 8 s .. 8 s + 7 of a result as the bf16 fragment of k-step s
__device__ __forceinline__ bf16x8 pack8(const float* v) {
  union { bf16x8 v; uint32_t u[4]; } f;
#pragma unroll
  for (int i = 0; i < 4; ++i) f.u[i] = pack2(v[2 * i], v[2 * i + 1]);
  return f.v;
}

// ---- staging: a tile of 32 rows x 64 bf16 is 256 x 16 bytes, thread `tid` moves row tid >> 3, columns 8 (tid & 7) .. + 7 ----
__device__ __forceinline__ uint4 fetch_bf16(const bf16_t* tile, int tid) { return reinterpret_cast<const uint4*>(tile)[tid]; }
// the same piece of an fp32 tile with row stride ld, rounded
__device__ __forceinline__ uint4 fetch_f32(const float* tile, int ld, int tid) {
  const float4* p = reinterpret_cast<const float4*>(tile + (size_t)(tid >> 3) * ld + 8 * (tid & 7));
  const float4 a = p[0], b = p[1];
  return make_uint4(pack2(a.x, a.y), pack2(a.z, a.w), pack2(b.x, b.y), pack2(b.z, b.w));
}
__device__ __forceinline__ void park_row(bf16_t* rowmajor, uint4 v, int tid) {
  *reinterpret_cast<uint4*>(rowmajor + (tid >> 3) * SA_RP + 8 * (tid & 7)) = v;
}
__device__ __forceinline__ void park_tr(bf16_t* transposed, uint4 v, int tid) {
  bf16_t* t = transposed + (8 * (tid & 7)) * SA_TP + (tid >> 3);
  const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    t[(2 * i) * SA_TP] = (bf16_t)(u[i] & 0xffffu);
    t[(2 * i + 1) * SA_TP] = (bf16_t)(u[i] >> 16);
  }
}

// fragments: A of a row-major tile (row = lane & 31, k-step s: columns 16 s + 8 (lane >> 5) .. + 7) ...
__device__ __forceinline__ bf16x8 frag_row(const bf16_t* rowmajor, int r, int h, int s) {
  return *reinterpret_cast<const bf16x8*>(rowmajor + r * SA_RP + 16 * s + 8 * h);
}
// ... and of a transposed tile (row d, k-step s over the swept rows, in the order of pack8)
__device__ __forceinline__ bf16x8 frag_tr(const bf16_t* transposed, int d, int h, int s) {
  union { bf16x8 v; bf16x4 q[2]; } f;
  const bf16_t* p = transposed + d * SA_TP + 16 * s + 4 * h;
  f.q[0] = *reinterpret_cast<const bf16x4*>(p);
  f.q[1] = *reinterpret_cast<const bf16x4*>(p + 8);
  return f.v;
}
// the wave's own 32 rows of a [Tp][64] bf16 operand as B fragments (column = lane & 31)
__device__ __forceinline__ void own_rows(bf16x8* f, const bf16_t* rows, int r, int h) {
#pragma unroll
  for (int s = 0; s < 4; ++s) f[s] = *reinterpret_cast<const bf16x8*>(rows + (size_t)r * 64 + 16 * s + 8 * h);
}

// out^T result (two 32 x 32 halves of d, column = the wave's row `r`) -> 64 fp32 columns of row `dst`, times f, or zeros
__device__ __forceinline__ void store_rows(float* dst, const floatx16& a0, const floatx16& a1, int h, float f, bool valid) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
    if (valid) {
      v0 = make_float4(a0[4 * g] * f, a0[4 * g + 1] * f, a0[4 * g + 2] * f, a0[4 * g + 3] * f);
      v1 = make_float4(a1[4 * g] * f, a1[4 * g + 1] * f, a1[4 * g + 2] * f, a1[4 * g + 3] * f);
    }
    *reinterpret_cast<float4*>(dst + 8 * g + 4 * h) = v0;
    *reinterpret_cast<float4*>(dst + 32 + 8 * g + 4 * h) = v1;
  }
}
// a workgroup whose 128 rows are all padding: zeros into its 128 x 64 piece of an fp32 tensor with row stride ld
__device__ __forceinline__ void zero_block(float* dst, int ld, int tid) {
  float4* p = reinterpret_cast<float4*>(dst + (size_t)(tid >> 1) * ld + 32 * (tid & 1));
#pragma unroll
  for (int i = 0; i < 8; ++i) p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

struct Who {  // blockIdx -> (row block, image, head)
  int blk, bh, b, hd;
  __device__ Who(int heads, int Tp) {
    const int nb = Tp / SA_Q;
    blk = blockIdx.x % nb;
    bh = blockIdx.x / nb;
    b = bh / heads;
    hd = bh - b * heads;
  }
};

// qkv fp32 [batch * Tp][3 C] -> o bf16 [3][batch * heads][Tp][64], the q third times log2(e) / 8; four elements per thread
__global__ __launch_bounds__(256) void s3_attn_prep_kernel(const float4* __restrict__ qkv, uint2* __restrict__ o, int heads, int Tp,
                                                           int64_t n4, int64_t plane) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int C = heads * 64, w4 = 3 * C / 4;
  const int64_t row = i / w4;
  const int col = (int)(i - row * w4) * 4, which = col / C, hc = col - which * C, hd = hc >> 6, d = hc & 63;
  const int64_t b = row / Tp, t = row - b * Tp;
  const float f = which == 0 ? SA_QSCALE : 1.0f;
  const float4 v = qkv[i];
  o[(which * plane + ((b * heads + hd) * Tp + t) * 64 + d) / 4] = make_uint2(pack2(v.x * f, v.y * f), pack2(v.z * f, v.w * f));
}

// ao[b Tp + q][64 hd ..] = softmax_k(q . k / 8) v over the keys < T, lse[bh Tp + q] = log2 sum_k 2^(q' . k); rows q >= T: 0, 0
__global__ __launch_bounds__(256) void s3_attn_fwd_kernel(const bf16_t* __restrict__ qkvb, float* __restrict__ ao,
                                                          float* __restrict__ lse, int heads, int T, int Tp, int64_t plane) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[2][SA_ROW];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[2][SA_TR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const Who w(heads, Tp);
  const int C = heads * 64, q0 = w.blk * SA_Q, q = q0 + wave * 32 + r;
  float* orow = ao + ((size_t)w.b * Tp + q0) * C + w.hd * 64;
  if (q0 >= T) {
    zero_block(orow, C, tid);
    if (tid < SA_Q) lse[(size_t)w.bh * Tp + q0 + tid] = 0.f;
    return;
  }
  const bf16_t* qp = qkvb + (size_t)w.bh * Tp * 64;
  const bf16_t *kp = qp + plane, *vp = kp + plane;
  bf16x8 qf[4];
  own_rows(qf, qp + (size_t)(q0 + wave * 32) * 64, r, h);
  floatx16 o0 = zero16(), o1 = zero16();
  float m = SA_NEG, l = 0.f;
  const int nt = (T + SA_T - 1) / SA_T;
  uint4 kr = fetch_bf16(kp, tid), vr = fetch_bf16(vp, tid);
  park_row(Ks[0], kr, tid);
  park_tr(Vt[0], vr, tid);
  __syncthreads();
  for (int kt = 0; kt < nt; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nt;
    if (more) {
      kr = fetch_bf16(kp + (size_t)(kt + 1) * SA_T * 64, tid);
      vr = fetch_bf16(vp + (size_t)(kt + 1) * SA_T * 64, tid);
    }
    floatx16 s = zero16();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_row(Ks[cur], r, h, ks), qf[ks], s, 0, 0, 0);
    float p[16], tmax = SA_NEG;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int key = kt * SA_T + (i & 3) + 8 * (i >> 2) + 4 * h;
      p[i] = key < T ? s[i] : SA_NEG;
      tmax = fmaxf(tmax, p[i]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));  // the query's other 16 keys of the tile
    const float m_new = fmaxf(m, tmax), alpha = __builtin_amdgcn_exp2f(m - m_new);
    float psum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      p[i] = __builtin_amdgcn_exp2f(p[i] - m_new);
      psum += p[i];
    }
    l = l * alpha + psum;  // this lane's keys only: the halves are added behind the loop (same m, same alpha)
    m = m_new;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      o0[i] *= alpha;
      o1[i] *= alpha;
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 pb = pack8(p + 8 * ks);
      o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Vt[cur], r, h, ks), pb, o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Vt[cur], 32 + r, h, ks), pb, o1, 0, 0, 0);
    }
    if (more) {
      park_row(Ks[cur ^ 1], kr, tid);
      park_tr(Vt[cur ^ 1], vr, tid);
    }
    __syncthreads();
  }
  l += __shfl_xor(l, 32, 64);
  const bool valid = q < T;
  store_rows(orow + (size_t)(wave * 32 + r) * C, o0, o1, h, 1.0f / l, valid);
  if (h == 0) lse[(size_t)w.bh * Tp + q] = valid ? m + log2f(l) : 0.f;
}

// dq (columns 64 hd .. of dqkv [batch * Tp][3 C]) of one block of 128 queries, sweeping the keys < T
__global__ __launch_bounds__(256) void s3_attn_dq_kernel(const bf16_t* __restrict__ qkvb, const float* __restrict__ dao,
                                                         const float* __restrict__ lse, const float* __restrict__ D,
                                                         float* __restrict__ dqkv, int heads, int T, int Tp, int64_t plane) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[2][SA_ROW];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[2][SA_ROW];
  __shared__ __attribute__((aligned(16))) bf16_t Kt[2][SA_TR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const Who w(heads, Tp);
  const int C = heads * 64, q0 = w.blk * SA_Q, q = q0 + wave * 32 + r;
  float* orow = dqkv + ((size_t)w.b * Tp + q0) * 3 * C + w.hd * 64;
  if (q0 >= T) {
    zero_block(orow, 3 * C, tid);
    return;
  }
  const bf16_t* qp = qkvb + (size_t)w.bh * Tp * 64;
  const bf16_t *kp = qp + plane, *vp = kp + plane;
  const bool valid = q < T;
  bf16x8 qf[4], dof[4];
  own_rows(qf, qp + (size_t)(q0 + wave * 32) * 64, r, h);
  {
    const float* dp = dao + ((size_t)w.b * Tp + q) * C + w.hd * 64 + 8 * h;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const float4 a = *reinterpret_cast<const float4*>(dp + 16 * ks), b = *reinterpret_cast<const float4*>(dp + 16 * ks + 4);
      const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      dof[ks] = pack8(v);
    }
  }
  const float lq = lse[(size_t)w.bh * Tp + q], Dq = D[(size_t)w.bh * Tp + q];
  floatx16 g0 = zero16(), g1 = zero16();
  const int nt = (T + SA_T - 1) / SA_T;
  uint4 kr = fetch_bf16(kp, tid), vr = fetch_bf16(vp, tid);
  park_row(Ks[0], kr, tid);
  park_tr(Kt[0], kr, tid);
  park_row(Vs[0], vr, tid);
  __syncthreads();
  for (int kt = 0; kt < nt; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nt;
    if (more) {
      kr = fetch_bf16(kp + (size_t)(kt + 1) * SA_T * 64, tid);
      vr = fetch_bf16(vp + (size_t)(kt + 1) * SA_T * 64, tid);
    }
    floatx16 s = zero16(), dp = zero16();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_row(Ks[cur], r, h, ks), qf[ks], s, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_row(Vs[cur], r, h, ks), dof[ks], dp, 0, 0, 0);
    }
    float ds[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int key = kt * SA_T + (i & 3) + 8 * (i >> 2) + 4 * h;
      const float p = __builtin_amdgcn_exp2f(s[i] - lq);
      ds[i] = (valid && key < T) ? p * (dp[i] - Dq) : 0.f;
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 db = pack8(ds + 8 * ks);
      g0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Kt[cur], r, h, ks), db, g0, 0, 0, 0);
      g1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Kt[cur], 32 + r, h, ks), db, g1, 0, 0, 0);
    }
    if (more) {
      park_row(Ks[cur ^ 1], kr, tid);
      park_tr(Kt[cur ^ 1], kr, tid);
      park_row(Vs[cur ^ 1], vr, tid);
    }
    __syncthreads();
  }
  store_rows(orow + (size_t)(wave * 32 + r) * 3 * C, g0, g1, h, 0.125f, valid);
}

// dk, dv (columns C + 64 hd .., 2 C + 64 hd .. of dqkv) of one block of 128 keys, sweeping the queries < T
__global__ __launch_bounds__(256) void s3_attn_dkv_kernel(const bf16_t* __restrict__ qkvb, const float* __restrict__ dao,
                                                          const float* __restrict__ lse, const float* __restrict__ D,
                                                          float* __restrict__ dqkv, int heads, int T, int Tp, int64_t plane) {
  __shared__ __attribute__((aligned(16))) bf16_t Qs[2][SA_ROW];
  __shared__ __attribute__((aligned(16))) bf16_t Os[2][SA_ROW];
  __shared__ __attribute__((aligned(16))) bf16_t Qt[2][SA_TR];
  __shared__ __attribute__((aligned(16))) bf16_t Ot[2][SA_TR];
  __shared__ float Ls[2][2][SA_T];  // [buffer][lse, D][query of the tile]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const Who w(heads, Tp);
  const int C = heads * 64, k0 = w.blk * SA_Q, key = k0 + wave * 32 + r;
  float* orow = dqkv + ((size_t)w.b * Tp + k0) * 3 * C + C + w.hd * 64;
  if (k0 >= T) {
    zero_block(orow, 3 * C, tid);
    zero_block(orow + C, 3 * C, tid);
    return;
  }
  const bf16_t* qp = qkvb + (size_t)w.bh * Tp * 64;
  const bf16_t *kp = qp + plane, *vp = kp + plane;
  const float* dop = dao + (size_t)w.b * Tp * C + w.hd * 64;
  const float *lp = lse + (size_t)w.bh * Tp, *Dp = D + (size_t)w.bh * Tp;
  const bool valid = key < T;
  bf16x8 kf[4], vf[4];
  own_rows(kf, kp + (size_t)(k0 + wave * 32) * 64, r, h);
  own_rows(vf, vp + (size_t)(k0 + wave * 32) * 64, r, h);
  floatx16 gk0 = zero16(), gk1 = zero16(), gv0 = zero16(), gv1 = zero16();
  const int nt = (T + SA_T - 1) / SA_T;
  uint4 qr = fetch_bf16(qp, tid), dr = fetch_f32(dop, C, tid);
  float st = tid < 64 ? (tid < 32 ? lp[tid] : Dp[tid - 32]) : 0.f;
  park_row(Qs[0], qr, tid);
  park_tr(Qt[0], qr, tid);
  park_row(Os[0], dr, tid);
  park_tr(Ot[0], dr, tid);
  if (tid < 64) Ls[0][tid >> 5][tid & 31] = st;
  __syncthreads();
  for (int qt = 0; qt < nt; ++qt) {
    const int cur = qt & 1;
    const bool more = qt + 1 < nt;
    if (more) {
      const int n0 = (qt + 1) * SA_T;
      qr = fetch_bf16(qp + (size_t)n0 * 64, tid);
      dr = fetch_f32(dop + (size_t)n0 * C, C, tid);
      if (tid < 64) st = tid < 32 ? lp[n0 + tid] : Dp[n0 + tid - 32];
    }
    floatx16 s = zero16(), dp = zero16();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_row(Qs[cur], r, h, ks), kf[ks], s, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_row(Os[cur], r, h, ks), vf[ks], dp, 0, 0, 0);
    }
    float p[16], ds[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int qi = (i & 3) + 8 * (i >> 2) + 4 * h;
      const float e = __builtin_amdgcn_exp2f(s[i] - Ls[cur][0][qi]);
      const bool on = valid && qt * SA_T + qi < T;
      p[i] = on ? e : 0.f;
      ds[i] = on ? e * (dp[i] - Ls[cur][1][qi]) : 0.f;
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 pb = pack8(p + 8 * ks), db = pack8(ds + 8 * ks);
      gv0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Ot[cur], r, h, ks), pb, gv0, 0, 0, 0);
      gv1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Ot[cur], 32 + r, h, ks), pb, gv1, 0, 0, 0);
      gk0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Qt[cur], r, h, ks), db, gk0, 0, 0, 0);
      gk1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Qt[cur], 32 + r, h, ks), db, gk1, 0, 0, 0);
    }
    if (more) {
      park_row(Qs[cur ^ 1], qr, tid);
      park_tr(Qt[cur ^ 1], qr, tid);
      park_row(Os[cur ^ 1], dr, tid);
      park_tr(Ot[cur ^ 1], dr, tid);
      if (tid < 64) Ls[cur ^ 1][tid >> 5][tid & 31] = st;
    }
    __syncthreads();
  }
  float* mine = orow + (size_t)(wave * 32 + r) * 3 * C;
  store_rows(mine, gk0, gk1, h, SA_LN2, valid);
  store_rows(mine + C, gv0, gv1, h, 1.0f, valid);
}

bool dims_ok(int batch, int heads, int T, int Tp) {
  return batch >= 1 && heads >= 1 && Tp >= SA_Q && Tp % SA_Q == 0 && T >= 1 && T <= Tp &&
         (int64_t)batch * Tp * heads * 3 <= 0x7fffffffLL;  // the grids, and the int row count of dvt_parts_rowdot
}

}  // namespace

extern "C" int64_t dvt_s3_attn_operand_bytes(int batch, int heads, int Tp) {
  if (batch < 1 || heads < 1 || Tp < 1) return -1;
  return (int64_t)3 * batch * heads * Tp * 64 * 2;
}

extern "C" int dvt_s3_attn_fwd(const float* qkv, void* qkvb, float* ao, float* lse, int batch, int heads, int T, int Tp,
                               void* stream) {
  if (!qkv || !qkvb || !ao || !lse || !dims_ok(batch, heads, T, Tp)) return DVT_E_BADARG;
  if (!dvt_aligned16(qkv) || !dvt_aligned16(qkvb) || !dvt_aligned16(ao)) return DVT_E_BADARG;
  const hipStream_t s = (hipStream_t)stream;
  const int64_t plane = (int64_t)batch * heads * Tp * 64, n4 = 3 * plane / 4;
  hipLaunchKernelGGL(s3_attn_prep_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, (const float4*)qkv, (uint2*)qkvb,
                     heads, Tp, n4, plane);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(s3_attn_fwd_kernel, dim3((unsigned)(batch * heads * (Tp / SA_Q))), dim3(256), 0, s, (const bf16_t*)qkvb, ao,
                     lse, heads, T, Tp, plane);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int dvt_s3_attn_bwd(const void* qkvb, const float* ao, const float* dao, const float* lse, float* D, float* dqkv,
                               int batch, int heads, int T, int Tp, void* stream) {
  if (!qkvb || !ao || !dao || !lse || !D || !dqkv || !dims_ok(batch, heads, T, Tp)) return DVT_E_BADARG;
  if (!dvt_aligned16(qkvb) || !dvt_aligned16(ao) || !dvt_aligned16(dao) || !dvt_aligned16(dqkv)) return DVT_E_BADARG;
  const hipStream_t s = (hipStream_t)stream;
  const int64_t plane = (int64_t)batch * heads * Tp * 64;
  const dim3 grid((unsigned)(batch * heads * (Tp / SA_Q))), blk(256);
  DVT_TRY(dvt_parts_rowdot(dao, ao, D, batch * Tp, Tp, heads * 64, stream));
  hipLaunchKernelGGL(s3_attn_dkv_kernel, grid, blk, 0, s, (const bf16_t*)qkvb, dao, lse, (const float*)D, dqkv, heads, T, Tp, plane);
  DVT_CHECK_LAUNCH();
  hipLaunchKernelGGL(s3_attn_dq_kernel, grid, blk, 0, s, (const bf16_t*)qkvb, dao, lse, (const float*)D, dqkv, heads, T, Tp, plane);
  DVT_CHECK_LAUNCH();
  return 0;
}
