// Stage-3 distillation step (include/dvt_stage3.h): forward, loss and backward of a whole DINOv2 ViT in exact fp32.
//
// Reference: main_distillation.py:85-296 (student PretrainedViTWrapper, loss, loop), timm 1.0.7 VisionTransformer
// (absent third party; forward restated in oracle/vit.py).
//
// The block is the stage-2 block with LayerScale: x1 = x + ls1 (.) proj(attn(norm1 x)), x2 = x1 + ls2 (.)
// fc2(gelu(fc1(norm2 x1))): block_fwd / block_bwd of dvt_block_train.hip, with every kernel they launch, the opt-in bf16
// linear layers included.  The patch embedding's im2col and the prefix-token / pos_embed assembly are the fp32 extractor's
// kernels (dvt_vit_f32.hip).  This file holds the step around them: the padded patch weight and its gradient, the pos_embed
// resample, the final norm, the loss over the patch rows, and the assembly's backward.
//
// Rows: an image owns s_pad rows (prefix tokens, then patches, then zero padding).  Padded rows are zero in every activation
// that feeds a reduction over rows, as in stage 2; the prefix rows take part in every block but not in the loss.
#include "dvt_common.h"
#include "dvt_block_train.h"
#include "dvt_row_dev.h"
#include "../../include/dvt_parts.h"
#include "../../include/dvt_stage2.h"
#include "../../include/dvt_stage3.h"

namespace {

// ==========================================================================================================
// Patch embedding: the im2col and the token assembly are the fp32 extractor's (dvt_im2col_f32, dvt_embed_f32 of
// dvt_vit_f32.hip); here the weight padded from [dim, 3 p p] to [dim, k_patch] (and its gradient back) and the assembly's
// backward.
// ==========================================================================================================
// wpad[n][k] = k < k0 ? w[n][k] : 0   (n rows, kp >= k0 columns)
__global__ __launch_bounds__(256) void s3_pad_kernel(const float* __restrict__ w, float* __restrict__ wpad, int n, int k0, int kp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)n * kp) return;
  const int r = (int)(i / kp), k = (int)(i - (int64_t)r * kp);
  wpad[i] = k < k0 ? w[(int64_t)r * k0 + k] : 0.f;
}

// g[n][k] += gpad[n][k] for k < k0
__global__ __launch_bounds__(256) void s3_unpad_add_kernel(const float* __restrict__ gpad, float* __restrict__ g, int n, int k0, int kp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)n * k0) return;
  const int r = (int)(i / k0), k = (int)(i - (int64_t)r * k0);
  g[i] += gpad[(int64_t)r * kp + k];
}

// Backward of the token assembly (embed_f32_kernel).  dx [batch * s_pad, dim] (the gradient w.r.t. the first block's input)
// in, per token row s and float4 column q:  dprefix[s] += sum_b dx[b, s]  (s < n_prefix),  dpos[row of s] += sum_b dx[b, s]  (the cls row when
// pos_has_cls, every patch row);  then dx's prefix rows are zeroed, so that dx is the patch-embedding output's gradient (its
// padded rows are zero already).  One thread owns (s, q) over the whole batch: no atomics, no races.
__global__ __launch_bounds__(256) void s3_embed_bwd_kernel(float4* __restrict__ dx, float4* __restrict__ dprefix,
                                                           float4* __restrict__ dpos, int batch, DvtVitConfig c) {
  const int dq = c.dim >> 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)c.n_tokens * dq) return;
  const int s = (int)(i / dq), q = (int)(i - (int64_t)s * dq);
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int b = 0; b < batch; ++b) sum = f4_add(sum, dx[((int64_t)b * c.s_pad + s) * dq + q]);
  if (s < c.n_prefix) {
    dprefix[(size_t)s * dq + q] = f4_add(dprefix[(size_t)s * dq + q], sum);
    if (c.pos_has_cls && s == 0) dpos[q] = f4_add(dpos[q], sum);
    for (int b = 0; b < batch; ++b) dx[((int64_t)b * c.s_pad + s) * dq + q] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    const size_t p = (size_t)(s - c.n_prefix + c.pos_has_cls) * dq + q;
    dpos[p] = f4_add(dpos[p], sum);
  }
}

// ==========================================================================================================
// pos_embed resample (timm resample_abs_pos_embed: F.interpolate(bicubic, antialias, align_corners=False) in fp32 on the
// square patch part of the table) and its transpose.  The map is linear and separable: per channel O = Wy P Wx^T with the
// host's tables Wy [gh, g0], Wx [gw, g0] (dvt_amd.s3.pos_tables takes them from torch itself).  All four passes -- x then y
// forward (ATen's order), y then x backward -- are one contraction along one axis of a [A, B, dim] map:
//   out[a, b, :] (+)= sum_k w[sel * wo + k * wk] * in[a * ia + b * ib + k * ik, :]      sel = a or b
// One wave owns 64 float4 columns of one output row: the table entry is the same for every lane (a scalar load), the map's
// rows are read and written as coalesced 16-byte columns.  k ascends, entries that are exactly zero (everything outside the
// filter's band) are skipped, one fma per tap: the order is fixed, nothing is atomic, two runs give the same bits.  A null
// table is the identity along its axis (the resize keeps that axis' length).  The block past the last row carries the cls
// row over when the table has one.
// ==========================================================================================================
struct PosPass {
  const float* w;      // the table, or nullptr for the identity (K == the selected axis' length)
  int A, B, K;         // output rows a < A, b < B; taps k < K
  int sel_b;           // the table row follows b (else a)
  int wo, wk;          // table index = sel * wo + k * wk
  int ia, ib, ik;      // input row = a * ia + b * ib + k * ik
  int dq;              // float4 columns per row (dim / 4)
};

template <bool ACC>
__global__ __launch_bounds__(64) void s3_pos_pass_kernel(const float4* __restrict__ in, float4* __restrict__ out,
                                                         const float4* __restrict__ cls_in, float4* __restrict__ cls_out,
                                                         PosPass p) {
  const int q = blockIdx.y * 64 + threadIdx.x;
  if (q >= p.dq) return;
  const int r = blockIdx.x;
  if (r == p.A * p.B) {  // the cls row (launched only when there is one)
    cls_out[q] = ACC ? f4_add(cls_out[q], cls_in[q]) : cls_in[q];
    return;
  }
  const int a = r / p.B, b = r - a * p.B, sel = p.sel_b ? b : a;
  const float4* src = in + ((size_t)a * p.ia + (size_t)b * p.ib) * p.dq + q;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (p.w) {
    const float* w = p.w + (size_t)sel * p.wo;
    for (int k = 0; k < p.K; ++k) {
      const float wk = w[(size_t)k * p.wk];
      if (wk == 0.f) continue;
      const float4 x = src[(size_t)k * p.ik * p.dq];
      acc = make_float4(fmaf(wk, x.x, acc.x), fmaf(wk, x.y, acc.y), fmaf(wk, x.z, acc.z), fmaf(wk, x.w, acc.w));
    }
  } else {
    acc = src[(size_t)sel * p.ik * p.dq];
  }
  float4* dst = out + (size_t)r * p.dq + q;
  *dst = ACC ? f4_add(*dst, acc) : acc;
}

template <bool ACC>
int pos_pass(const float* in, float* out, const float* cls_in, float* cls_out, const PosPass& p, hipStream_t s) {
  const dim3 grid(p.A * p.B + (cls_in ? 1 : 0), dvt_cdiv(p.dq, 64));
  hipLaunchKernelGGL(s3_pos_pass_kernel<ACC>, grid, dim3(64), 0, s, (const float4*)in, (float4*)out, (const float4*)cls_in,
                     (float4*)cls_out, p);
  DVT_CHECK_LAUNCH();
  return 0;
}

// wy may be null only when g0 == gh, wx only when g0 == gw
int pos_check(const float* wy, const float* wx, int g0, int gh, int gw, int dim, int has_cls) {
  if (g0 < 1 || gh < 1 || gw < 1 || dim < 4 || dim % 4 || (has_cls != 0 && has_cls != 1)) return DVT_E_BADARG;
  if ((!wy && g0 != gh) || (!wx && g0 != gw)) return DVT_E_BADARG;
  return 0;
}

// pos [has_cls + g0 g0, dim] -> out [has_cls + gh gw, dim]; tmp [g0, gw, dim]
int pos_resample_fwd(const float* pos, float* out, const float* wy, const float* wx, float* tmp, int g0, int gh, int gw,
                     int dim, int has_cls, hipStream_t s) {
  const int dq = dim / 4, c = has_cls * dim;
  // x pass: T[p, j] = sum_q Wx[j, q] P[p, q]
  DVT_TRY(pos_pass<false>(pos + c, tmp, nullptr, nullptr, PosPass{wx, g0, gw, g0, 1, g0, 1, g0, 0, 1, dq}, s));
  // y pass: O[i, j] = sum_p Wy[i, p] T[p, j]
  return pos_pass<false>(tmp, out + c, has_cls ? pos : nullptr, out, PosPass{wy, gh, gw, g0, 0, g0, 1, 0, 1, gw, dq}, s);
}

// dout [has_cls + gh gw, dim] -> dpos [has_cls + g0 g0, dim] += its transpose; tmp [g0, gw, dim]
int pos_resample_bwd(const float* dout, float* dpos, const float* wy, const float* wx, float* tmp, int g0, int gh, int gw,
                     int dim, int has_cls, hipStream_t s) {
  const int dq = dim / 4, c = has_cls * dim;
  // dT[p, j] = sum_i Wy[i, p] dO[i, j]
  DVT_TRY(pos_pass<false>(dout + c, tmp, nullptr, nullptr, PosPass{wy, g0, gw, gh, 0, 1, g0, 0, 1, gw, dq}, s));
  // dP[p, q] += sum_j Wx[j, q] dT[p, j]: a gather down the table's column q
  return pos_pass<true>(tmp, dpos + c, has_cls ? dout : nullptr, dpos, PosPass{wx, g0, g0, gw, 1, 1, g0, gw, 0, 1, dq}, s);
}

// ---- host side ------------------------------------------------------------------------------------------
enum { PATCHW = 0, PATCHB, CLS, REG, POS, BLK0 };

int check_cfg(const DvtVitConfig* c) {
  if (!c) return DVT_E_BADARG;
  if (c->dim != 384 && c->dim != 768 && c->dim != 1024) return DVT_E_BADARG;
  if (c->heads * 64 != c->dim || c->mlp_dim <= 0 || c->mlp_dim % 128) return DVT_E_BADARG;
  if (c->depth < 1 || c->depth > DVT_VIT_MAX_DEPTH || c->patch < 1 || c->stride < 1) return DVT_E_BADARG;
  if (c->grid_h < 1 || c->grid_w < 1 || (c->grid_h - 1) * c->stride + c->patch > c->img_h ||
      (c->grid_w - 1) * c->stride + c->patch > c->img_w)
    return DVT_E_BADARG;
  if (c->n_prefix < 1 || c->n_tokens != c->n_prefix + c->grid_h * c->grid_w) return DVT_E_BADARG;
  if (c->s_pad < c->n_tokens || c->s_pad % 128) return DVT_E_BADARG;
  if (c->k_patch < 3 * c->patch * c->patch || c->k_patch % 32) return DVT_E_BADARG;
  if ((c->pos_has_cls != 0 && c->pos_has_cls != 1) || !(c->ln_eps > 0.f)) return DVT_E_BADARG;
  return 0;
}

int64_t n_offsets(const DvtVitConfig* c) { return 8 + (int64_t)DVT_S3_TENSORS_PER_BLOCK * c->depth; }

// out[0 .. n_offsets - 1] as include/dvt_stage3.h lays it out; g0 > 0: pos_embed keeps the checkpoint's g0 x g0 grid
void offsets(const DvtVitConfig* c, int64_t* out, int g0 = 0) {
  const int64_t C = c->dim, F = c->mlp_dim, pk = 3LL * c->patch * c->patch;
  int64_t at = 0, i = 0;
  auto put = [&](int64_t floats) {
    out[i++] = at;
    at += (floats + 3) / 4 * 4;  // 16-byte boundaries
  };
  put(C * pk);
  put(C);
  put(C);
  put((int64_t)(c->n_prefix - 1) * C);
  put((int64_t)(c->pos_has_cls + (g0 > 0 ? g0 * g0 : c->grid_h * c->grid_w)) * C);
  const int64_t sz[DVT_S3_TENSORS_PER_BLOCK] = {C, C, 3 * C * C, 3 * C, C * C, C, C, C, C, F * C, F, C * F, C, C};
  for (int b = 0; b < c->depth; ++b)
    for (int t = 0; t < DVT_S3_TENSORS_PER_BLOCK; ++t) put(sz[t]);
  put(C);
  put(C);
  out[i] = at;
}

struct S3Work {
  BlockActs blk[DVT_VIT_MAX_DEPTH];
  float *xl, *xf, *meanf, *rstdf;  // the last block's output and its final norm
  float *col, *wpad, *dwpad, *emb;
  BlockScratch g;
  float *pos, *dpos, *ptmp;  // the run-grid position table, its gradient and the resample's [g0, gw, dim] intermediate
  BlockBf16 bf[DVT_VIT_MAX_DEPTH];  // gemm_mode bit 1: per block the bf16 weight copies, and the one A-operand scratch in each;
                                    // bit 2: the block's bf16 attention operands and lse too; bit 4: the weight gradient's scratch
};

// gemm_mode (include/dvt_stage3.h): the bit set MODE_GEMM | MODE_ATTN | MODE_WGRAD of dvt_block_train.h
bool mode_ok(int mode) { return block_mode_ok(mode); }

// the table's grid differs from the run's: the step resamples pos_embed on its way in and its gradient on the way out
bool resamples(const DvtVitConfig* c, int g0) { return g0 > 0 && (g0 != c->grid_h || g0 != c->grid_w); }

int64_t carve(const DvtVitConfig* c, int batch, char* base, S3Work* w, int g0 = 0, int mode = 0) {
  const int64_t R = (int64_t)batch * c->s_pad, C = c->dim, F = c->mlp_dim;
  // mode 3 keeps neither P nor a block's fp32 qkv: every block's qkv is the backward's dqkv scratch, idle during the forward
  const int64_t PP = (mode & MODE_ATTN) ? 0 : (int64_t)batch * c->heads * c->s_pad * c->s_pad;
  Carver cv{base};
  S3Work t{};
  for (int b = 0; b < c->depth; ++b) carve_block_acts(cv, &t.blk[b], R, C, F, PP, true, !(mode & MODE_ATTN));
  t.xl = cv.take(R * C);
  t.xf = cv.take(R * C);
  t.meanf = cv.take(R);
  t.rstdf = cv.take(R);
  t.col = cv.take(R * c->k_patch);
  t.wpad = cv.take(C * c->k_patch);
  t.dwpad = cv.take(C * c->k_patch);
  t.emb = cv.take(R * C);
  carve_block_scratch(cv, &t.g, R, C, F, PP, (int64_t)batch * c->heads * c->s_pad);
  if (mode & MODE_ATTN)
    for (int b = 0; b < c->depth; ++b) t.blk[b].qkv = t.g.dqkv;
  if (resamples(c, g0)) {  // behind everything else: the equal-grid workspace is what it always was
    const int64_t n = (int64_t)(c->pos_has_cls + c->grid_h * c->grid_w) * C;
    t.pos = cv.take(n);
    t.dpos = cv.take(n);
    t.ptmp = cv.take((int64_t)g0 * c->grid_w * C);
  }
  // behind everything else again: the fp32 mode's sizes and carving are what they were
  carve_block_bf16(cv, t.bf, c->depth, R, C, F, (int64_t)batch * c->heads * c->s_pad, mode);
  if (w) *w = t;
  return cv.o;
}

int run(const DvtVitConfig* c, const float* params, float* grads, const float* img, const float* target, float* feat,
        int batch, int norm_batch, void* work, int64_t work_bytes, float* loss_out, hipStream_t s, int g0 = 0,
        const float* wy = nullptr, const float* wx = nullptr, int mode = 0) {
  DVT_TRY(check_cfg(c));
  if (!mode_ok(mode)) return DVT_E_BADARG;
  const bool rs = resamples(c, g0);
  if (rs) DVT_TRY(pos_check(wy, wx, g0, c->grid_h, c->grid_w, c->dim, c->pos_has_cls));
  if (!params || !grads || !img || !target || !loss_out || !work || batch < 1 || norm_batch < batch) return DVT_E_BADARG;
  S3Work w;
  if (carve(c, batch, reinterpret_cast<char*>(work), &w, g0, mode) > work_bytes) return DVT_E_BADARG;
  if ((mode & MODE_GEMM) && (!dvt_aligned16(params) || !dvt_aligned16(work))) return DVT_E_BADARG;  // (the casts move 16-byte pieces)
  int64_t po[8 + DVT_S3_TENSORS_PER_BLOCK * DVT_VIT_MAX_DEPTH];
  offsets(c, po, g0);
  const int C = c->dim, F = c->mlp_dim, T = c->n_tokens, Tp = c->s_pad, NB = c->depth;
  const int K0 = 3 * c->patch * c->patch, KP = c->k_patch;
  const int R = batch * Tp;
  const BlockDims bd{{batch, c->heads, T, Tp, C}, F, c->ln_eps};
  auto P = [&](int b) { return block_tensors(params, po + BLK0 + DVT_S3_TENSORS_PER_BLOCK * b, true); };
  auto mp = [&](int b) { return (mode & MODE_GEMM) ? &w.bf[b] : nullptr; };
  const int64_t normw = po[BLK0 + DVT_S3_TENSORS_PER_BLOCK * NB], normb = po[BLK0 + DVT_S3_TENSORS_PER_BLOCK * NB + 1];
  if (mode & MODE_GEMM)  // the weights of this call, rounded once: `params` changes between steps, and a slice is a step's unit
    for (int b = 0; b < NB; ++b) DVT_TRY(cast_block_weights(P(b), w.bf[b], C, F, s));

  // ---- forward: patch embedding, token assembly, block 0's norm1 ----
  {
    const int64_t n = (int64_t)C * KP;
    hipLaunchKernelGGL(s3_pad_kernel, dim3(dvt_cdiv(n, 256)), dim3(256), 0, s, params + po[PATCHW], w.wpad, C, K0, KP);
    DVT_CHECK_LAUNCH();
  }
  DVT_TRY(dvt_im2col_f32(img, w.col, *c, R, s));
  DVT_TRY(lin_fwd(w.col, w.wpad, params + po[PATCHB], w.emb, R, C, KP, s));
  if (rs) DVT_TRY(pos_resample_fwd(params + po[POS], w.pos, wy, wx, w.ptmp, g0, c->grid_h, c->grid_w, C, c->pos_has_cls, s));
  DVT_TRY(dvt_embed_f32(w.emb, w.blk[0].xin, params + po[CLS], rs ? w.pos : params + po[POS], *c, R, s));
  DVT_TRY(ls_add_ln(C, w.blk[0].xin, nullptr, nullptr, nullptr, P(0).n1w, P(0).n1b, w.blk[0].xn1, w.blk[0].mean1,
                    w.blk[0].rstd1, T, Tp, R, c->ln_eps, s));
  // ---- the blocks (s_pad % 128 == 0: always the attention-row kernel, forward and dS; bits 3 and 4 of dvt_tune_set(18, .)
  // are stage 2's), each followed by its LayerScale residual add fused with the next block's norm1, or the final norm ----
  for (int b = 0; b < NB; ++b) {
    const BlockActs& k = w.blk[b];
    DVT_TRY(block_fwd(bd, P(b), k, mp(b), true, s));
    if (b + 1 < NB) {
      const BlockActs& n = w.blk[b + 1];
      DVT_TRY(resid_ln(C, k.x1, k.f2, P(b).ls2, n.xin, P(b + 1).n1w, P(b + 1).n1b, n.xn1, n.mean1, n.rstd1, T, Tp, R,
                       c->ln_eps, s));
    } else {
      DVT_TRY(resid_ln(C, k.x1, k.f2, P(b).ls2, w.xl, params + normw, params + normb, w.xf, w.meanf, w.rstdf, T, Tp, R,
                       c->ln_eps, s));
    }
  }

  // ---- loss over the patch rows ----
  DVT_TRY(loss_rows(false, C, w.xf, nullptr, target, feat, w.g.d1, w.g.acc, c->n_prefix, T, Tp, R, norm_batch, loss_out, s));
  // final norm: d0 = d xl
  DVT_TRY(ln_bwd(C, w.g.d1, w.xl, w.meanf, w.rstdf, params + normw, nullptr, w.g.d0, grads + normw, grads + normb, R, s));

  // ---- backward: d0 holds the gradient w.r.t. the current block's OUTPUT ----
  for (int b = NB - 1; b >= 0; --b)
    DVT_TRY(block_bwd(bd, P(b), block_tensors(grads, po + BLK0 + DVT_S3_TENSORS_PER_BLOCK * b, true), w.blk[b], w.g, mp(b),
                      true, true, s));
  // ---- token assembly and patch embedding ----
  {
    if (rs) {  // the assembly's backward adds into a zeroed run-grid gradient; the transpose pass adds that into `grads`
      const hipError_t e = hipMemsetAsync(w.dpos, 0, sizeof(float) * (size_t)(c->pos_has_cls + c->grid_h * c->grid_w) * C, s);
      if (e != hipSuccess) return (int)e;
    }
    const int64_t n = (int64_t)T * (C / 4);
    hipLaunchKernelGGL(s3_embed_bwd_kernel, dim3(dvt_cdiv(n, 256)), dim3(256), 0, s, (float4*)w.g.d0, (float4*)(grads + po[CLS]),
                       (float4*)(rs ? w.dpos : grads + po[POS]), batch, *c);
    DVT_CHECK_LAUNCH();
    if (rs) DVT_TRY(pos_resample_bwd(w.dpos, grads + po[POS], wy, wx, w.ptmp, g0, c->grid_h, c->grid_w, C, c->pos_has_cls, s));
  }
  {
    const hipError_t e = hipMemsetAsync(w.dwpad, 0, sizeof(float) * (size_t)C * KP, s);
    if (e != hipSuccess) return (int)e;
  }
  DVT_TRY(lin_bwd(w.g.d0, w.col, w.wpad, nullptr, w.dwpad, grads + po[PATCHB], R, C, KP, s));
  {
    const int64_t n = (int64_t)C * K0;
    hipLaunchKernelGGL(s3_unpad_add_kernel, dim3(dvt_cdiv(n, 256)), dim3(256), 0, s, (const float*)w.dwpad, grads + po[PATCHW],
                       C, K0, KP);
    DVT_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

extern "C" int dvt_s3_param_offsets(const DvtVitConfig* cfg, int64_t* out) {
  if (!out) return DVT_E_BADARG;
  DVT_TRY(check_cfg(cfg));
  offsets(cfg, out);
  return 0;
}

extern "C" int64_t dvt_s3_workspace_bytes(const DvtVitConfig* cfg, int batch) {
  if (check_cfg(cfg) != 0 || batch < 1) return -1;
  return carve(cfg, batch, nullptr, nullptr);
}

extern "C" int dvt_s3_train_slice(const DvtVitConfig* cfg, const float* params, float* grads, const float* img,
                                  const float* target, float* feat_out, int batch, int norm_batch, void* work,
                                  int64_t work_bytes, float* loss_out, void* stream) {
  return run(cfg, params, grads, img, target, feat_out, batch, norm_batch, work, work_bytes, loss_out, (hipStream_t)stream);
}

extern "C" int dvt_s3_train_step(const DvtVitConfig* cfg, const float* params, float* grads, const float* img,
                                 const float* target, float* feat_out, int batch, void* work, int64_t work_bytes,
                                 float* loss_out, void* stream) {
  return run(cfg, params, grads, img, target, feat_out, batch, batch, work, work_bytes, loss_out, (hipStream_t)stream);
}

// ---- another position grid (include/dvt_stage3.h) ---------------------------------------------------------
extern "C" int dvt_pos_resample_fwd(const float* pos, float* out, const float* wy, const float* wx, float* tmp, int g0,
                                    int grid_h, int grid_w, int dim, int has_cls, void* stream) {
  DVT_TRY(pos_check(wy, wx, g0, grid_h, grid_w, dim, has_cls));
  if (!pos || !out || !tmp || !dvt_aligned16(pos) || !dvt_aligned16(out) || !dvt_aligned16(tmp)) return DVT_E_BADARG;
  return pos_resample_fwd(pos, out, wy, wx, tmp, g0, grid_h, grid_w, dim, has_cls, (hipStream_t)stream);
}

extern "C" int dvt_pos_resample_bwd(const float* dout, float* dpos, const float* wy, const float* wx, float* tmp, int g0,
                                    int grid_h, int grid_w, int dim, int has_cls, void* stream) {
  DVT_TRY(pos_check(wy, wx, g0, grid_h, grid_w, dim, has_cls));
  if (!dout || !dpos || !tmp || !dvt_aligned16(dout) || !dvt_aligned16(dpos) || !dvt_aligned16(tmp)) return DVT_E_BADARG;
  return pos_resample_bwd(dout, dpos, wy, wx, tmp, g0, grid_h, grid_w, dim, has_cls, (hipStream_t)stream);
}

extern "C" int dvt_s3_param_offsets_pos(const DvtVitConfig* cfg, int g0, int64_t* out) {
  if (!out || g0 < 1) return DVT_E_BADARG;
  DVT_TRY(check_cfg(cfg));
  offsets(cfg, out, g0);
  return 0;
}

extern "C" int64_t dvt_s3_workspace_bytes_pos(const DvtVitConfig* cfg, int batch, int g0) {
  if (check_cfg(cfg) != 0 || batch < 1 || g0 < 1) return -1;
  return carve(cfg, batch, nullptr, nullptr, g0);
}

extern "C" int64_t dvt_s3_workspace_bytes_mp(const DvtVitConfig* cfg, int batch, int g0, int gemm_mode) {
  if (check_cfg(cfg) != 0 || batch < 1 || g0 < 0 || !mode_ok(gemm_mode)) return -1;
  return carve(cfg, batch, nullptr, nullptr, g0, gemm_mode);
}

extern "C" int dvt_s3_train_slice_pos_mp(const DvtVitConfig* cfg, int g0, const float* wy, const float* wx, int gemm_mode,
                                         const float* params, float* grads, const float* img, const float* target,
                                         float* feat_out, int batch, int norm_batch, void* work, int64_t work_bytes,
                                         float* loss_out, void* stream) {
  if (g0 < 0 || !mode_ok(gemm_mode)) return DVT_E_BADARG;
  return run(cfg, params, grads, img, target, feat_out, batch, norm_batch, work, work_bytes, loss_out, (hipStream_t)stream, g0,
             wy, wx, gemm_mode);
}

extern "C" int dvt_s3_train_slice_pos(const DvtVitConfig* cfg, int g0, const float* wy, const float* wx, const float* params,
                                      float* grads, const float* img, const float* target, float* feat_out, int batch,
                                      int norm_batch, void* work, int64_t work_bytes, float* loss_out, void* stream) {
  if (g0 < 1) return DVT_E_BADARG;
  return run(cfg, params, grads, img, target, feat_out, batch, norm_batch, work, work_bytes, loss_out, (hipStream_t)stream, g0,
             wy, wx);
}

// ---- component entry points for tests (include/dvt_parts.h): forwarders to the kernels above; no kernel and no launch of their
// own, every check in front of the launch ----
namespace {
// the fields the assembly / im2col kernels read, the rest zero
int parts_cfg(DvtVitConfig* c, int dim, int n_prefix, int n_tokens, int s_pad, int pos_has_cls) {
  if (dim < 4 || (dim & 3) || n_prefix < 0 || n_tokens <= n_prefix || s_pad < n_tokens || (pos_has_cls != 0 && pos_has_cls != 1))
    return DVT_E_BADARG;
  *c = DvtVitConfig{};
  c->dim = dim;
  c->n_prefix = n_prefix;
  c->n_tokens = n_tokens;
  c->s_pad = s_pad;
  c->pos_has_cls = pos_has_cls;
  return 0;
}
}  // namespace

extern "C" int dvt_parts_s3_embed(const float* y, float* x, const float* prefix, const float* pos, int batch, int dim, int n_prefix,
                                  int n_tokens, int s_pad, int pos_has_cls, void* stream) {
  DvtVitConfig c;
  DVT_TRY(parts_cfg(&c, dim, n_prefix, n_tokens, s_pad, pos_has_cls));
  if (!y || !x || !pos || (n_prefix > 0 && !prefix) || batch < 1 || !dvt_aligned16(y) || !dvt_aligned16(x) || !dvt_aligned16(prefix) || !dvt_aligned16(pos))
    return DVT_E_BADARG;
  return dvt_embed_f32(y, x, prefix, pos, c, batch * s_pad, (hipStream_t)stream);
}

extern "C" int dvt_parts_s3_embed_bwd(float* dx, float* dprefix, float* dpos, int batch, int dim, int n_prefix, int n_tokens,
                                      int s_pad, int pos_has_cls, void* stream) {
  DvtVitConfig c;
  DVT_TRY(parts_cfg(&c, dim, n_prefix, n_tokens, s_pad, pos_has_cls));
  if (!dx || !dpos || (n_prefix > 0 && !dprefix) || batch < 1 || !dvt_aligned16(dx) || !dvt_aligned16(dprefix) || !dvt_aligned16(dpos))
    return DVT_E_BADARG;
  const int64_t n = (int64_t)n_tokens * (dim / 4);
  hipLaunchKernelGGL(s3_embed_bwd_kernel, dim3(dvt_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (float4*)dx, (float4*)dprefix,
                     (float4*)dpos, batch, c);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int dvt_parts_s3_im2col(const float* img, float* col, int batch, int patch, int stride, int img_h, int img_w, int grid_h,
                                   int grid_w, int n_prefix, int s_pad, int k_patch, void* stream) {
  if (!img || !col || batch < 1 || patch < 1 || stride < 1 || grid_h < 1 || grid_w < 1 || n_prefix < 0) return DVT_E_BADARG;
  if ((grid_h - 1) * stride + patch > img_h || (grid_w - 1) * stride + patch > img_w) return DVT_E_BADARG;
  if (s_pad < n_prefix + grid_h * grid_w || k_patch < 3 * patch * patch) return DVT_E_BADARG;
  DvtVitConfig c{};
  c.patch = patch;
  c.stride = stride;
  c.img_h = img_h;
  c.img_w = img_w;
  c.grid_h = grid_h;
  c.grid_w = grid_w;
  c.n_prefix = n_prefix;
  c.n_tokens = n_prefix + grid_h * grid_w;
  c.s_pad = s_pad;
  c.k_patch = k_patch;
  return dvt_im2col_f32(img, col, c, batch * s_pad, (hipStream_t)stream);
}
