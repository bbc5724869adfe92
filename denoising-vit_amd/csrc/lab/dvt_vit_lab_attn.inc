// lab/dvt_vit_lab_attn.inc -- the round-2 attention loop ("v1": S -> softmax -> P.V strictly in sequence, tile max reduced
// every tile), superseded by attention_kernel_v2 in round 3 (+10 %).  Included by dvt_vit_attn.hip inside its anonymous namespace
// under -DDVT_LAB only (dvt_tune_set(1, -501) of libdvt_hip_lab.so); shares KV_TILE / VT_LD / ATT_Q with the product kernel.
__global__ __launch_bounds__(512) void attention_kernel(const bf16_t* __restrict__ qk,
                                                        const bf16_t* __restrict__ vt,
                                                        bf16_t* __restrict__ out, int heads,
                                                        int s_pad, int n_valid) {
  // two K / V^T tile buffers: tile kt+1 is written while tile kt is being multiplied, one barrier per tile
  __shared__ __attribute__((aligned(16))) char Ksb[2][KV_TILE * 128];
  __shared__ __attribute__((aligned(16))) char Vsb[2][64 * VT_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, lc = lane & 15;
  // 1-D grid; XCD x gets a contiguous run of (image, head, query-block) triples so that the
  // query blocks of one head share that XCD's L2 copy of K / V^T (round-robin placement would
  // spread them over all 8 L2s: 8x the K/V traffic)
  const int nqb = s_pad / ATT_Q;
  int id = blockIdx.x;
  {
    const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = id & 7, loc = id >> 3;
    id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  }
  const int qb = id % nqb, h = (id / nqb) % heads, b = id / (nqb * heads);
  const int dim = heads * 64, ldq = 2 * dim;
  const size_t row0 = (size_t)b * s_pad;

  // Q fragments (B operand of S^T = K.Q^T): lane column = query lc, k = d = 32*ks + 8*g + j.
  // Pre-scaled by head_dim^-0.5 = 0.125 (exact in bf16).
  bf16x8 qf[2];
  {
    const bf16_t* qrow = qk + (row0 + qb * ATT_Q + wave * 16 + lc) * ldq + h * 64;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      union { bf16x8 v; uint32_t u[4]; } raw;
      raw.v = *reinterpret_cast<const bf16x8*>(qrow + ks * 32 + g * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float lo = __uint_as_float(raw.u[j] << 16) * 0.125f;
        const float hi = __uint_as_float(raw.u[j] & 0xffff0000u) * 0.125f;
        raw.u[j] = pack2(lo, hi);
      }
      qf[ks] = raw.v;
    }
  }
  const bf16_t* kbase = qk + row0 * ldq + dim + h * 64;
  const bf16_t* vbase = vt + ((size_t)(b * heads + h) * 64) * s_pad;

  f32x4 o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m_run = -1e30f, l_run = 0.f;  // running max / partial sum (this lane's keys only)
  const float LOG2E = 1.4426950408889634f;

  const int ntiles = (n_valid + KV_TILE - 1) / KV_TILE;
  // register-staged K / V^T tiles: one 16-B chunk per thread per operand (512 chunks each)
  const int sr0 = tid >> 3, sc = tid & 7;
  const bf16_t* kp0 = kbase + (size_t)sr0 * ldq + sc * 8;
  const bf16_t* vp0 = vbase + (size_t)sr0 * s_pad + sc * 8;
  const int kdo = sr0 * 128 + ((sc ^ (sr0 & 7)) << 4);
  // this thread's 8 keys 8 sc .. 8 sc + 7 of V^T row sr0: k-step sc >> 2, c = sc & 3 -> half (c >> 1) of the
  // chunks of lane groups g = 2 (c & 1) (first 4 keys) and g + 1 (last 4 keys)
  const int vks = sc >> 2, vc = sc & 3, vsw = (sr0 >> 1) & 7;
  const int vdo0 = sr0 * VT_LD + (((vks * 4 + 2 * (vc & 1)) ^ vsw) << 4) + (vc >> 1) * 8;
  const int vdo1 = sr0 * VT_LD + (((vks * 4 + 2 * (vc & 1) + 1) ^ vsw) << 4) + (vc >> 1) * 8;
  uint4 kr0, vr0;
#define ATT_LOAD(kt)                                                                   \
  do {                                                                                 \
    kr0 = *reinterpret_cast<const uint4*>(kp0 + (size_t)(kt) * KV_TILE * ldq);         \
    vr0 = *reinterpret_cast<const uint4*>(vp0 + (kt) * KV_TILE);                       \
  } while (0)
#define ATT_STORE(b)                                      \
  do {                                                    \
    *reinterpret_cast<uint4*>(Ksb[b] + kdo) = kr0;        \
    *reinterpret_cast<uint2*>(Vsb[b] + vdo0) = make_uint2(vr0.x, vr0.y); \
    *reinterpret_cast<uint2*>(Vsb[b] + vdo1) = make_uint2(vr0.z, vr0.w); \
  } while (0)
  ATT_LOAD(0);
  ATT_STORE(0);
  if (ntiles > 1) ATT_LOAD(1);
  __syncthreads();
  for (int kt = 0; kt < ntiles; ++kt) {
    const char* Ks = Ksb[kt & 1];
    const char* Vs = Vsb[kt & 1];
    if (kt + 1 < ntiles) {
      ATT_STORE((kt + 1) & 1);  // loaded during the previous tile; that buffer's readers passed the last barrier
      if (kt + 2 < ntiles) ATT_LOAD(kt + 2);
    }
    // ---- S^T[key][q] = K . Q^T : acc s[mt][r] <-> key = 16*mt + 4*g + r, q = lc
    f32x4 s[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      s[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int krow = mt * 16 + lc;
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + krow * 128 + (((ks * 4 + g) ^ (krow & 7)) << 4));
        s[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], s[mt], 0, 0, 0);
      }
    }
    // ---- online softmax over keys (a query's 64 keys live in the 4 lanes {lc + 16*g})
    const int kbase_idx = kt * KV_TILE;
    if (kt == ntiles - 1) {  // only the last tile can contain padding keys (wave-uniform branch)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (kbase_idx + mt * 16 + 4 * g + r >= n_valid) s[mt][r] = -1e30f;
    }
    // 16 values per lane: v_max3_f32 tree (8 instructions)
    float tmax = __builtin_fmaxf(__builtin_fmaxf(s[0][0], s[0][1]), s[0][2]);
    tmax = max3f(tmax, s[0][3], s[1][0]);
    tmax = max3f(tmax, s[1][1], s[1][2]);
    tmax = max3f(tmax, s[1][3], s[2][0]);
    tmax = max3f(tmax, s[2][1], s[2][2]);
    tmax = max3f(tmax, s[2][3], s[3][0]);
    tmax = max3f(tmax, s[3][1], s[3][2]);
    tmax = fmaxf(tmax, s[3][3]);
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m_run, tmax);
    // v_exp_f32 directly: arguments are <= 0, results in [0, 1]; a flushed denormal is an exact 0
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E);
    const float mb = m_new * LOG2E;
    // packed fp32 math (v_pk_fma_f32 / v_pk_add_f32): two logits per instruction
    const f32x2 l2e2 = {LOG2E, LOG2E}, nmb2 = {-mb, -mb};
    f32x2 ps2 = {0.f, 0.f};
    float pv[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const f32x2 sv = {s[mt][2 * h2], s[mt][2 * h2 + 1]};
        const f32x2 t = __builtin_elementwise_fma(sv, l2e2, nmb2);
        f32x2 e;
        e.x = __builtin_amdgcn_exp2f(t.x);
        e.y = __builtin_amdgcn_exp2f(t.y);
        ps2 += e;
        pv[mt][2 * h2] = e.x;
        pv[mt][2 * h2 + 1] = e.y;
      }
    const float psum = ps2.x + ps2.y;
    // B operand of O^T = V^T.P^T: k slot j = 4*(mt&1) + r of k-step ks = mt>>1
    union { bf16x8 v; uint32_t u[4]; } pf0, pf1;
    pf0.u[0] = pack2(pv[0][0], pv[0][1]); pf0.u[1] = pack2(pv[0][2], pv[0][3]);
    pf0.u[2] = pack2(pv[1][0], pv[1][1]); pf0.u[3] = pack2(pv[1][2], pv[1][3]);
    pf1.u[0] = pack2(pv[2][0], pv[2][1]); pf1.u[1] = pack2(pv[2][2], pv[2][3]);
    pf1.u[2] = pack2(pv[3][0], pv[3][1]); pf1.u[3] = pack2(pv[3][2], pv[3][3]);
    l_run = l_run * alpha + psum;
    if (!__all(m_new == m_run)) {  // wave-uniform: the running max rarely moves after the first tiles
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o[i][0] *= alpha;
        o[i][1] *= alpha;
        o[i][2] *= alpha;
        o[i][3] *= alpha;
      }
    }
    m_run = m_new;
    // ---- O^T[d][q] += V^T . P^T : A rows = d (16*mt + lc), k slots <-> keys 32*ks + 16*(j>>2) + 4*g + (j&3)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int vr = mt * 16 + lc, vs_ = (vr >> 1) & 7;
      const char* vrow = Vs + vr * VT_LD;
      const bf16x8 vf0 = *reinterpret_cast<const bf16x8*>(vrow + ((g ^ vs_) << 4));
      const bf16x8 vf1 = *reinterpret_cast<const bf16x8*>(vrow + (((4 + g) ^ vs_) << 4));
      o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf0, pf0.v, o[mt], 0, 0, 0);
      o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf1, pf1.v, o[mt], 0, 0, 0);
    }
    __syncthreads();  // tile kt+1 is complete in LDS, everyone is done reading tile kt
  }
#undef ATT_LOAD
#undef ATT_STORE
  // total row sum across the 4 key groups of the query
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  const float inv = 1.0f / l_run;
  // o[mt][r] = O[q = lc][d = 16*mt + 4*g + r]
  bf16_t* orow = out + (row0 + qb * ATT_Q + wave * 16 + lc) * dim + h * 64;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    uint2 pk;
    pk.x = pack2(o[mt][0] * inv, o[mt][1] * inv);
    pk.y = pack2(o[mt][2] * inv, o[mt][3] * inv);
    *reinterpret_cast<uint2*>(orow + mt * 16 + 4 * g) = pk;
  }
}

// ---- host side of the developer build's attention: its knobs, its share of the two attention entry points and of
// dvt_tune_set(1, v).  The product functions of dvt_vit_attn.hip call these through one guarded line each.
int g_vit_attn_l2_mask = ATT_L2_VAR;  // dvt_tune_set(1, -540 - x): the product's mask (559 = 1 + 2 + 4 + 8 + 32 + 512) with the bits x toggled: 2 = P.V
                                      // fragment by fragment, 512 = no group pattern for the K reads, 514 = both, 128 / 256 / 384 = ablations (idle
                                      // waves compute / whole tail tile / both)
int g_vit_attn_variant = 2;  // dvt_tune_set(1, -500 - v): 2 (default) = attention_kernel_v2, 1 = the round-2 kernel

// dvt_vit_attention_log2q, in front of the product's launch: true = another build of the log2-domain kernel is selected and
// took the launch (*rc: its status, DVT_E_BADARG for a mask no build exists for); false = the product's mask
bool lab_launch_attention_l2(const void* qk, const void* vt, void* out, int heads, int s_pad, int n_valid, const dim3 grid,
                             hipStream_t stream, int* rc) {
  if (g_vit_attn_l2_mask == ATT_L2_VAR) return false;
  {  // ablation builds / the other P.V order
#define A2L_VAR(n)                                                                                                    \
  if (g_vit_attn_l2_mask == (n)) {                                                                                    \
    hipLaunchKernelGGL(attention_kernel_l2<(n)>, grid, dim3(512), 0, (hipStream_t)stream, (const bf16_t*)qk,          \
                       (const bf16_t*)vt, (bf16_t*)out, heads, s_pad, n_valid);                                       \
    *rc = (int)hipGetLastError();                                                                                     \
    return true;                                                                                                      \
  }
    A2L_VAR(ATT_L2_VAR ^ 2) A2L_VAR(ATT_L2_VAR ^ 128) A2L_VAR(ATT_L2_VAR ^ 256) A2L_VAR(ATT_L2_VAR ^ 384) A2L_VAR(ATT_L2_VAR ^ 512)
    A2L_VAR(ATT_L2_VAR ^ 514) A2L_VAR(ATT_L2_VAR ^ 1024) A2L_VAR(ATT_L2_VAR ^ 2048) A2L_VAR(ATT_L2_VAR ^ 4096) A2L_VAR(ATT_L2_VAR ^ 8192) A2L_VAR(ATT_L2_VAR ^ 16384) A2L_VAR(ATT_L2_VAR ^ 32768) A2L_VAR(ATT_L2_VAR ^ (32768 + 65536))
#undef A2L_VAR
    *rc = DVT_E_BADARG;
    return true;
  }
}

// whether the product's kernel and schedule mask are the selected ones (the forward pre-scales q only then)
bool lab_attn_product_selected() { return g_vit_attn_variant == 2 && g_vit_attn_mask == 15; }

// dvt_vit_attention, in front of the product's launch (attention_kernel_v2<15>): the round-2 kernel or another schedule mask
bool lab_launch_attention(const void* qk, const void* vt, void* out, int heads, int s_pad, int n_valid, const dim3 grid,
                          hipStream_t stream, int* rc) {
  if (lab_attn_product_selected()) return false;
  if (g_vit_attn_variant != 2) {
    *rc = DVT_E_BADARG;
    if (s_pad % ATT_Q) return true;  // (the round-2 loop has no query-block tail)
    hipLaunchKernelGGL(attention_kernel, grid, dim3(512), 0, (hipStream_t)stream, (const bf16_t*)qk, (const bf16_t*)vt,
                       (bf16_t*)out, heads, s_pad, n_valid);
    *rc = (int)hipGetLastError();
    return true;
  }
  bool done = false;
#define A2_VAR(n)                                                                                                     \
  if (g_vit_attn_mask == n) {                                                                                         \
    hipLaunchKernelGGL(attention_kernel_v2<n>, grid, dim3(512), 0, (hipStream_t)stream, (const bf16_t*)qk,            \
                       (const bf16_t*)vt, (bf16_t*)out, heads, s_pad, n_valid);                                       \
    done = true;                                                                                                      \
  }
  A2_VAR(0) A2_VAR(1) A2_VAR(2) A2_VAR(4) A2_VAR(8) A2_VAR(16) A2_VAR(64) A2_VAR(3) A2_VAR(31) A2_VAR(79)
#undef A2_VAR
  *rc = done ? (int)hipGetLastError() : DVT_E_BADARG;
  return true;
}

// vit_attn_tune, behind -530 / -531.  dvt_vit_tune asks attention BEFORE the GEMM, whose -700 - pct (0 .. 400) would
// otherwise take -540 - 256 / 384 / 512 / 514.  The reverse case: -540 - 128 and -540 - 1024 ... -540 - 32768 lie in the 4w
// GEMM's grid keys (-600 - n, -1100 - n), which the decoder has always asked first -- they set that grid, never reached
// the list below, and are therefore not in it (attention_kernel_l2 builds of those masks exist, unselectable, as before).
int lab_attn_tune(int v) {
  if (v == -540 || v == -540 - 2 || v == -540 - 256 || v == -540 - 384 || v == -540 - 512 || v == -540 - 514 || v == -540 - 32768 - 65536) {
    g_vit_attn_l2_mask = ATT_L2_VAR ^ (-540 - v);
    return 0;
  }
  if (v <= -510 && v > -530) {
    g_vit_attn_mask = -510 - v;
    return 0;
  }
  if (v == -510 - 31 || v == -510 - 64 || v == -510 - 79) {
    g_vit_attn_mask = -510 - v;
    return 0;
  }
  if (v == -501 || v == -502) {
    g_vit_attn_variant = -500 - v;
    return 0;
  }
  return VIT_TUNE_NOT_MINE;
}
