// Stage-2 generalizable denoiser: forward, loss, backward and AdamW of
// `Denoiser` = pos_embed + num_blocks x timm Block on [batch, 1369, 768] feature maps.
//
// Reference: dvt/models/online_denoiser.py:13-104 (model), main_denoiser.py:204-221 (one step),
// timm 1.0.7 vision_transformer.Block / Attention / Mlp (absent third party; restated in oracle/stage2.py).
//
// Everything is exact fp32, like the reference.  The contractions -- linear layers forward / data gradient /
// weight gradient, and the four attention products per direction -- all go through ONE GEMM kernel family
// (dvt_gemm_f32_ex, v_mfma_f32_32x32x2_f32 behind a 3-stage LDS-DMA pipeline).  The block -- its forward and backward launch
// sequences and every kernel they run but the two unfused softmax passes -- is dvt_block_train.hip's, which the stage-3 step
// runs as well; this file holds the step around the blocks (input add + norm, unpack or loss, pos_embed gradient), the
// softmax passes, AdamW and the process's A/B switches.  Attention keeps its probabilities P [batch*heads, Tp, Tp]
// in HBM: at 288 GB per GPU the 3 GB that costs at batch 32 is cheaper than recomputing QK^T in the backward
// pass, and P is exactly what dV = P^T dO and dS = P (dP - rowsum(P dP)) need.
//
// Rows: an image owns tokens_pad rows; rows t >= tokens are all-zero in every activation that feeds a
// reduction over rows (xn, dY), so weight gradients and LayerNorm parameter gradients never see them; key
// columns >= tokens get probability 0.
#include <cstdlib>
#include "dvt_common.h"
#include "dvt_block_train.h"
#include "dvt_tune.h"
#include "dvt_row_dev.h"
#include "../../include/dvt_parts.h"
#include "../../include/dvt_stage2.h"

int g_s2_fork_wgrad = 1;  // DVT_S2_FORK_WGRAD=0 / dvt_tune_set(18, mask) bit 5: weight gradients on the caller's stream (A/B)
int g_s2_attn_rows = 1;  // DVT_S2_ATTN_ROWS=0: the [Tp][Tp] products on the 64 x 64 GEMM tile + separate softmax passes (A/B)
int g_s2_fuse_softmax_bwd = 1;  // DVT_S2_FUSE_SOFTMAX_BWD=0: dP written, s2_softmax_bwd_kernel over it (A/B)
int g_s2_big_wgrad = 1;  // DVT_S2_BIG_WGRAD=0: the weight-gradient GEMMs on the 64 x 64 tile (A/B)
int g_s2_big_bwd = 1;  // DVT_S2_BIG_BWD=0: the data-gradient GEMMs on the 64 x 64 tile (A/B)
int g_s2_big_fwd = 1;  // DVT_S2_BIG=0 in the environment of the process: the 64 x 64 tile for the forward layers too (A/B)

namespace {

// pred[batch, T, C] = a + b (padded rows in, packed rows out): the last residual add of an inference forward
template <int C>
__global__ __launch_bounds__(256) void s2_add_unpack_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            float* __restrict__ pred, int T, int Tp, int R) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int img = r / Tp, t = r - img * Tp;
  if (t >= T) return;
  Row<C> x, y;
  x.load(a + (size_t)r * C, lane);
  y.load(b + (size_t)r * C, lane);
  ROW_FOR(j, Row<C>::NJ) x.v[j] = f4_add(x.v[j], y.v[j]);
  x.store(pred + ((size_t)img * T + t) * C, lane);
}

// ==========================================================================================================
// softmax over the valid keys of one row of S [batch*heads*Tp rows][Tp], in place:  P = softmax(scale * S).
// One wave per row, two passes (online max / sum, then normalise).  Query rows >= T and key columns >= T: 0.
// timm Attention: q * scale, attn = q @ k^T, softmax(dim=-1).
// ==========================================================================================================
__global__ __launch_bounds__(256) void s2_softmax_kernel(float* __restrict__ S, int T, int Tp, int64_t rows, float scale) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float4* row = reinterpret_cast<float4*>(S + r * Tp);
  const int q = (int)(r % Tp), n4 = Tp / 4;
  if (q >= T) {
    for (int i = lane; i < n4; i += 64) row[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  float m = -3.0e38f, l = 0.f;
  for (int i = lane; i < n4; i += 64) {
    const float4 v = row[i];
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (4 * i + c < T) {
        const float s = e[c] * scale;
        const float mn = fmaxf(m, s);
        l = l * __expf(m - mn) + __expf(s - mn);
        m = mn;
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), l2 = __shfl_xor(l, o, 64);
    const float mn = fmaxf(m, m2);
    l = l * __expf(m - mn) + l2 * __expf(m2 - mn);
    m = mn;
  }
  const float inv = 1.0f / l;
  for (int i = lane; i < n4; i += 64) {
    const float4 v = row[i];
    float4 p;
    p.x = (4 * i + 0 < T) ? __expf(v.x * scale - m) * inv : 0.f;
    p.y = (4 * i + 1 < T) ? __expf(v.y * scale - m) * inv : 0.f;
    p.z = (4 * i + 2 < T) ? __expf(v.z * scale - m) * inv : 0.f;
    p.w = (4 * i + 3 < T) ? __expf(v.w * scale - m) * inv : 0.f;
    row[i] = p;
  }
}

// dS = scale * P * (dP - sum_k P dP), in place over dP (the gradient w.r.t. q k^T before the scale)
__global__ __launch_bounds__(256) void s2_softmax_bwd_kernel(const float* __restrict__ P, float* __restrict__ dP, int Tp,
                                                             int64_t rows, float scale) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float4* p = reinterpret_cast<const float4*>(P + r * Tp);
  float4* d = reinterpret_cast<float4*>(dP + r * Tp);
  const int n4 = Tp / 4;
  float dot = 0.f;
  for (int i = lane; i < n4; i += 64) dot += f4_dot(p[i], d[i]);
  dot = wave_sum(dot);
  for (int i = lane; i < n4; i += 64) {
    const float4 pv = p[i], dv = d[i];
    d[i] = make_float4(scale * pv.x * (dv.x - dot), scale * pv.y * (dv.y - dot), scale * pv.z * (dv.z - dot),
                       scale * pv.w * (dv.w - dot));
  }
}

// dpos[t, c] += sum over images of dx[img * Tp + t, c]   (pos_embed broadcasts over the batch)
__global__ __launch_bounds__(256) void s2_pos_grad_kernel(const float4* __restrict__ dx, float4* __restrict__ dpos, int batch,
                                                          int T, int Tp, int C4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)T * C4) return;
  const int t = (int)(i / C4), c = (int)(i - (int64_t)t * C4);
  float4 s = dpos[i];
  for (int b = 0; b < batch; ++b) s = f4_add(s, dx[((int64_t)b * Tp + t) * C4 + c]);
  dpos[i] = s;
}

// torch.optim.AdamW (decoupled weight decay), fused gradient scaling and zero_grad
__global__ __launch_bounds__(256) void s2_adamw_kernel(float4* __restrict__ p, float4* __restrict__ g, float4* __restrict__ m,
                                                       float4* __restrict__ v, int64_t n4, float lr, float b1, float b2,
                                                       float eps, float wd, float step_size, float inv_sqrt_bc2,
                                                       float gscale) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 gv = g[i];
  float4 pv = p[i], mv = m[i], vv = v[i];
  const float decay = 1.0f - lr * wd;
#define S2_ADAMW(c)                                                        \
  do {                                                                     \
    const float gg = gv.c * gscale;                                        \
    pv.c *= decay;                                                         \
    mv.c = b1 * mv.c + (1.0f - b1) * gg;                                   \
    vv.c = b2 * vv.c + (1.0f - b2) * gg * gg;                              \
    pv.c -= step_size * (mv.c / (sqrtf(vv.c) * inv_sqrt_bc2 + eps));       \
  } while (0)
  S2_ADAMW(x);
  S2_ADAMW(y);
  S2_ADAMW(z);
  S2_ADAMW(w);
#undef S2_ADAMW
  p[i] = pv;
  m[i] = mv;
  v[i] = vv;
  g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- host side ------------------------------------------------------------------------------------------
struct S2Offsets {
  int64_t pos;
  int64_t t[DVT_S2_MAX_BLOCKS][DVT_S2_TENSORS_PER_BLOCK];
  int64_t total;
};

int check_cfg(const DvtS2Config* c) {
  if (!c) return DVT_E_BADARG;
  if (c->dim != 384 && c->dim != 768 && c->dim != 1024) return DVT_E_BADARG;
  if (c->heads * 64 != c->dim || c->mlp_dim <= 0 || c->mlp_dim % 64) return DVT_E_BADARG;
  if (c->tokens < 1 || c->tokens_pad < c->tokens || c->tokens_pad % 64) return DVT_E_BADARG;
  if (c->n_blocks < 1 || c->n_blocks > DVT_S2_MAX_BLOCKS || !(c->ln_eps > 0.f)) return DVT_E_BADARG;
  return 0;
}

void offsets(const DvtS2Config* c, S2Offsets* o) {
  const int64_t C = c->dim, F = c->mlp_dim;
  int64_t at = 0;
  o->pos = 0;
  if (c->enable_pe) at += (int64_t)c->tokens * C;
  const int64_t sz[DVT_S2_TENSORS_PER_BLOCK] = {C, C, 3 * C * C, 3 * C, C * C, C, C, C, F * C, F, C * F, C};
  for (int b = 0; b < c->n_blocks; ++b)
    for (int i = 0; i < DVT_S2_TENSORS_PER_BLOCK; ++i) {
      o->t[b][i] = at;
      at += sz[i];
    }
  o->total = at;
}

struct S2Work {
  BlockActs blk[DVT_S2_MAX_BLOCKS];
  BlockScratch g;  // training; inference with several blocks: d0 alone, the ping-pong partner of blk[0].xin
  float* tmp;      // f1 and f2 of every block: without LayerScale no gradient reads them
  BlockBf16 bf[DVT_S2_MAX_BLOCKS];  // gemm_mode (include/dvt_stage2.h) != 0: what dvt_block_train.h's carve_block_bf16 lays out
};

// gemm_mode != 0 (training only): the bf16 kernels walk 128-row tiles of an image's rows and of the mlp columns
bool mode_shape_ok(const DvtS2Config* c, int mode) { return mode == 0 || (c->tokens_pad % 128 == 0 && c->mlp_dim % 128 == 0); }

int64_t carve(const DvtS2Config* c, int batch, int training, char* base, S2Work* w, int mode = 0) {
  const int64_t R = (int64_t)batch * c->tokens_pad, C = c->dim, F = c->mlp_dim;
  // with the flash attention neither P nor dP nor a block's fp32 qkv is kept: every block's qkv is the backward's dqkv
  // scratch, idle during the forward (as in the stage-3 step)
  const int64_t PP = (mode & MODE_ATTN) ? 0 : (int64_t)batch * c->heads * c->tokens_pad * c->tokens_pad;
  Carver cv{base};
  S2Work t{};
  const int nb = training ? c->n_blocks : 1;
  for (int b = 0; b < nb; ++b) carve_block_acts(cv, &t.blk[b], R, C, F, PP, false, !(mode & MODE_ATTN));
  for (int b = nb; b < c->n_blocks; ++b) t.blk[b] = t.blk[0];  // inference: every block reuses one set
  if (!training && c->n_blocks > 1) t.g.d0 = cv.take(R * C);   // ping-pong partner of blk[0].xin
  t.tmp = cv.take(R * C);
  if (training) carve_block_scratch(cv, &t.g, R, C, F, PP, (int64_t)batch * c->heads * c->tokens_pad);
  for (int b = 0; b < c->n_blocks; ++b) t.blk[b].f1 = t.blk[b].f2 = t.tmp;
  if (training) {
    if (mode & MODE_ATTN)
      for (int b = 0; b < c->n_blocks; ++b) t.blk[b].qkv = t.g.dqkv;
    // behind everything else: mode 0's sizes and carving are what they were
    carve_block_bf16(cv, t.bf, c->n_blocks, R, C, F, (int64_t)batch * c->heads * c->tokens_pad, mode);
  }
  if (w) *w = t;
  return cv.o;
}

int run(const DvtS2Config* c, const float* params, float* grads, const float* x, const float* target, float* pred,
        int batch, void* work, int64_t work_bytes, float* loss_out, hipStream_t s, int mode = 0) {
  DVT_TRY(check_cfg(c));
  const int training = grads != nullptr;
  if (!params || !x || batch < 1 || !work || (training && (!target || !loss_out)) || (!training && !pred)) return DVT_E_BADARG;
  if (!block_mode_ok(mode) || (mode && !training) || !mode_shape_ok(c, mode)) return DVT_E_BADARG;
  if (mode && (!dvt_aligned16(params) || !dvt_aligned16(work))) return DVT_E_BADARG;  // (the casts move 16-byte pieces)
  S2Work w;
  if (carve(c, batch, training, reinterpret_cast<char*>(work), &w, mode) > work_bytes) return DVT_E_BADARG;
  S2Offsets po;
  offsets(c, &po);
  const int C = c->dim, T = c->tokens, Tp = c->tokens_pad, NB = c->n_blocks;
  const int R = batch * Tp;
  const bool attn_rows = g_s2_attn_rows && Tp % AR_Q == 0;  // s2_attn_rows_kernel walks whole blocks of 128 query rows
  const BlockDims bd{{batch, c->heads, T, Tp, C}, c->mlp_dim, c->ln_eps};
  auto P = [&](int b) { return block_tensors(params, po.t[b], false); };
  auto xin = [&](int b) {  // inference with several blocks: block inputs ping-pong
    return training ? w.blk[b].xin : (b & 1) ? w.g.d0 : w.blk[0].xin;
  };
  auto mp = [&](int b) { return (mode & MODE_GEMM) ? &w.bf[b] : nullptr; };
  if (mode & MODE_GEMM)  // the weights of this call, rounded once: `params` changes between steps
    for (int b = 0; b < NB; ++b) DVT_TRY(cast_block_weights(P(b), w.bf[b], C, c->mlp_dim, s));

  // ---- forward ----
  DVT_TRY(add_ln(C, x, 1, c->enable_pe ? params + po.pos : nullptr, 1, w.blk[0].xin, P(0).n1w, P(0).n1b, w.blk[0].xn1,
                 w.blk[0].mean1, w.blk[0].rstd1, T, Tp, R, c->ln_eps, s));
  for (int b = 0; b < NB; ++b) {
    BlockActs k = w.blk[b];
    k.xin = xin(b);
    DVT_TRY(block_fwd(bd, P(b), k, mp(b), attn_rows, s));
    if (b + 1 < NB) {
      const BlockActs& n = w.blk[b + 1];
      DVT_TRY(resid_ln(C, k.x1, k.f2, nullptr, xin(b + 1), P(b + 1).n1w, P(b + 1).n1b, n.xn1, n.mean1, n.rstd1, T, Tp, R,
                       c->ln_eps, s));
    }
  }
  const BlockActs& last = w.blk[NB - 1];
  if (!training) {
    switch (C) {
      case 384: return launch_rows(s2_add_unpack_kernel<384>, R, s, (const float*)last.x1, (const float*)w.tmp, pred, T, Tp, R);
      case 768: return launch_rows(s2_add_unpack_kernel<768>, R, s, (const float*)last.x1, (const float*)w.tmp, pred, T, Tp, R);
      default: return launch_rows(s2_add_unpack_kernel<1024>, R, s, (const float*)last.x1, (const float*)w.tmp, pred, T, Tp, R);
    }
  }

  // ---- loss ----
  DVT_TRY(loss_rows(true, C, last.x1, w.tmp, target, pred, w.g.d0, w.g.acc, 0, T, Tp, R, batch, loss_out, s));

  // ---- backward: d0 holds the gradient w.r.t. the current block's OUTPUT ----
  for (int b = NB - 1; b >= 0; --b)
    DVT_TRY(block_bwd(bd, P(b), block_tensors(grads, po.t[b], false), w.blk[b], w.g, mp(b), attn_rows,
                      g_s2_fuse_softmax_bwd != 0, s));
  if (c->enable_pe) {
    const int64_t n = (int64_t)T * (C / 4);
    hipLaunchKernelGGL(s2_pos_grad_kernel, dim3(dvt_cdiv(n, 256)), dim3(256), 0, s, (const float4*)w.g.d0,
                       (float4*)(grads + po.pos), batch, T, Tp, C / 4);
    DVT_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

extern "C" int dvt_s2_param_offsets(const DvtS2Config* cfg, int64_t* out) {
  if (!out) return DVT_E_BADARG;
  DVT_TRY(check_cfg(cfg));
  S2Offsets o;
  offsets(cfg, &o);
  out[0] = o.pos;
  for (int b = 0; b < cfg->n_blocks; ++b)
    for (int i = 0; i < DVT_S2_TENSORS_PER_BLOCK; ++i) out[1 + DVT_S2_TENSORS_PER_BLOCK * b + i] = o.t[b][i];
  out[1 + DVT_S2_TENSORS_PER_BLOCK * cfg->n_blocks] = o.total;
  return 0;
}

extern "C" int64_t dvt_s2_workspace_bytes(const DvtS2Config* cfg, int batch, int training) {
  if (check_cfg(cfg) != 0 || batch < 1) return -1;
  return carve(cfg, batch, training, nullptr, nullptr);
}

// dvt_tune_set(18, mask): the same switches from inside a process (tests / A/B tools): bit 0 forward layers, 1 data gradients,
// 2 weight gradients on the 128 x 128 tile, 3 softmax fused into the attention products, 4 softmax backward without a dP pass,
// 5 weight gradients on a side stream beside the data gradients; 63 = default.  Results differ in summation order only.
int dvt_s2_tune(int mask) {
  if (mask < 0 || mask > 63) return DVT_E_BADARG;
  s2_read_env();  // (so that a later first call does not overwrite this)
  g_s2_big_fwd = mask & 1;
  g_s2_big_bwd = (mask >> 1) & 1;
  g_s2_big_wgrad = (mask >> 2) & 1;
  g_s2_attn_rows = (mask >> 3) & 1;
  g_s2_fuse_softmax_bwd = (mask >> 4) & 1;
  g_s2_fork_wgrad = (mask >> 5) & 1;
  return 0;
}

void s2_read_env() {
  static bool done = false;
  if (done) return;
  done = true;
  const char* e = getenv("DVT_S2_BIG");
  if (e && e[0] == '0') g_s2_big_fwd = 0;
  e = getenv("DVT_S2_BIG_BWD");
  if (e && e[0] == '0') g_s2_big_bwd = 0;
  e = getenv("DVT_S2_FORK_WGRAD");
  if (e && e[0] == '0') g_s2_fork_wgrad = 0;
  e = getenv("DVT_S2_ATTN_ROWS");
  if (e && e[0] == '0') g_s2_attn_rows = 0;
  e = getenv("DVT_S2_FUSE_SOFTMAX_BWD");
  if (e && e[0] == '0') g_s2_fuse_softmax_bwd = 0;
  e = getenv("DVT_S2_BIG_WGRAD");
  if (e && e[0] == '0') g_s2_big_wgrad = 0;
}

extern "C" int dvt_s2_forward(const DvtS2Config* cfg, const float* params, const float* x, float* pred, int batch,
                              void* work, int64_t work_bytes, void* stream) {
  s2_read_env();
  return run(cfg, params, nullptr, x, nullptr, pred, batch, work, work_bytes, nullptr, (hipStream_t)stream);
}

extern "C" int dvt_s2_train_step(const DvtS2Config* cfg, const float* params, float* grads, const float* x,
                                 const float* target, float* pred, int batch, void* work, int64_t work_bytes,
                                 float* loss_out, void* stream) {
  s2_read_env();
  if (!grads) return DVT_E_BADARG;
  return run(cfg, params, grads, x, target, pred, batch, work, work_bytes, loss_out, (hipStream_t)stream);
}

extern "C" int64_t dvt_s2_workspace_bytes_mp(const DvtS2Config* cfg, int batch, int training, int gemm_mode) {
  if (check_cfg(cfg) != 0 || batch < 1 || !block_mode_ok(gemm_mode) || !mode_shape_ok(cfg, gemm_mode)) return -1;
  if (gemm_mode && !training) return -1;  // (bf16 inference is Denoiser(inference_dtype="bfloat16"), not this forward)
  return carve(cfg, batch, training, nullptr, nullptr, gemm_mode);
}

extern "C" int dvt_s2_train_step_mp(const DvtS2Config* cfg, const float* params, float* grads, const float* x,
                                    const float* target, float* pred, int batch, void* work, int64_t work_bytes,
                                    float* loss_out, void* stream, int gemm_mode) {
  s2_read_env();
  if (!grads || !block_mode_ok(gemm_mode)) return DVT_E_BADARG;
  return run(cfg, params, grads, x, target, pred, batch, work, work_bytes, loss_out, (hipStream_t)stream, gemm_mode);
}

extern "C" int dvt_adamw_step(float* params, float* grads, float* m, float* v, int64_t n, float lr, float beta1,
                              float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream) {
  if (!params || !grads || !m || !v || n <= 0 || (n & 3) || step < 1) return DVT_E_BADARG;
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  const float step_size = (float)(lr / bc1), inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  const int64_t n4 = n / 4;
  hipLaunchKernelGGL(s2_adamw_kernel, dim3(dvt_cdiv(n4, 256)), dim3(256), 0, (hipStream_t)stream, (float4*)params,
                     (float4*)grads, (float4*)m, (float4*)v, n4, lr, beta1, beta2, eps, weight_decay, step_size,
                     inv_sqrt_bc2, grad_scale);
  DVT_CHECK_LAUNCH();
  return 0;
}

// the two softmax passes of the unfused attention branches (dvt_block_train.h)
int s2_softmax(float* S, int T, int Tp, int64_t rows, float scale, hipStream_t s) {
  hipLaunchKernelGGL(s2_softmax_kernel, dim3(dvt_cdiv(rows, 4)), dim3(256), 0, s, S, T, Tp, rows, scale);
  DVT_CHECK_LAUNCH();
  return 0;
}

int s2_softmax_bwd(const float* P, float* dP, int Tp, int64_t rows, float scale, hipStream_t s) {
  hipLaunchKernelGGL(s2_softmax_bwd_kernel, dim3(dvt_cdiv(rows, 4)), dim3(256), 0, s, P, dP, Tp, rows, scale);
  DVT_CHECK_LAUNCH();
  return 0;
}

// ---- component entry points for tests (include/dvt_parts.h): forwarders to the kernels above; no kernel and no launch of
// their own, every check in front of the first launch ----
extern "C" int dvt_parts_softmax(const float* P, float* S, int T, int Tp, int64_t rows, float scale, int backward, void* stream) {
  if (!S || Tp < 4 || (Tp & 3) || T < 1 || T > Tp || rows < 1 || !dvt_aligned16(S) || (backward != 0 && backward != 1)) return DVT_E_BADARG;
  if (backward && (!P || !dvt_aligned16(P))) return DVT_E_BADARG;
  return backward ? s2_softmax_bwd(P, S, Tp, rows, scale, (hipStream_t)stream) : s2_softmax(S, T, Tp, rows, scale, (hipStream_t)stream);
}

extern "C" int dvt_parts_pos_grad(const float* dx, float* dpos, int batch, int T, int Tp, int C, void* stream) {
  if (!dx || !dpos || batch < 1 || T < 1 || Tp < T || C < 4 || (C & 3) || !dvt_aligned16(dx) || !dvt_aligned16(dpos)) return DVT_E_BADARG;
  const int64_t n = (int64_t)T * (C / 4);
  hipLaunchKernelGGL(s2_pos_grad_kernel, dim3(dvt_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)dx, (float4*)dpos,
                     batch, T, Tp, C / 4);
  DVT_CHECK_LAUNCH();
  return 0;
}
