// Stage-3 distillation step (include/dvt_stage3.h): forward, loss and backward of a whole DINOv2 ViT in exact fp32.
//
// Reference: main_distillation.py:85-296 (student PretrainedViTWrapper, loss, loop), timm 1.0.7 VisionTransformer
// (absent third party; forward restated in oracle/vit.py).
//
// The block is the stage-2 block (dvt_stage2.hip) with LayerScale: x1 = x + ls1 (.) proj(attn(norm1 x)), x2 = x1 + ls2 (.)
// fc2(gelu(fc1(norm2 x1))).  Contractions, attention, GELU and the LayerNorm backward are the stage-2 pieces
// (dvt_block_train.hip); this file adds the patch embedding (im2col + GEMM, padded weight), the prefix-token / pos_embed assembly,
// the LayerScale residual add fused with the following LayerNorm (the next block's norm1, or the final norm), the LayerScale
// backward, the loss over the patch rows, and the assembly's backward.
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
// Patch embedding: im2col of the image (one row per token row; prefix and padded rows zero) and the weight padded from
// [dim, 3 p p] to [dim, k_patch] (and its gradient back).
// ==========================================================================================================
__global__ __launch_bounds__(256) void s3_im2col_kernel(const float* __restrict__ img, float* __restrict__ col, DvtVitConfig c) {
  const int t = blockIdx.x;  // token row in [0, batch * s_pad)
  const int b = t / c.s_pad, s = t - b * c.s_pad;
  float* dst = col + (size_t)t * c.k_patch;
  const int pp = c.patch * c.patch;
  if (s < c.n_prefix || s >= c.n_tokens) {
    for (int k = threadIdx.x; k < c.k_patch; k += 256) dst[k] = 0.f;
    return;
  }
  const int py = (s - c.n_prefix) / c.grid_w, px = (s - c.n_prefix) - py * c.grid_w;
  const float* src = img + (size_t)b * 3 * c.img_h * c.img_w;
  for (int k = threadIdx.x; k < c.k_patch; k += 256) {
    float v = 0.f;
    if (k < 3 * pp) {
      const int ch = k / pp, rem = k - ch * pp, ky = rem / c.patch, kx = rem - ky * c.patch;
      v = src[((size_t)ch * c.img_h + py * c.stride + ky) * c.img_w + px * c.stride + kx];
    }
    dst[k] = v;
  }
}

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

// x[t] = prefix token (+ pos_embed[0] for cls when the table has a cls row) | patch embedding + pos_embed | 0 (padding)
// (timm VisionTransformer._pos_embed; oracle/vit.py:forward_features)
__global__ __launch_bounds__(256) void s3_embed_kernel(const float4* __restrict__ y, float4* __restrict__ x,
                                                       const float4* __restrict__ prefix, const float4* __restrict__ pos,
                                                       DvtVitConfig c) {
  const int t = blockIdx.x, s = t % c.s_pad, dq = c.dim >> 2;
  for (int q = threadIdx.x; q < dq; q += 256) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s < c.n_prefix) {
      o = prefix[(size_t)s * dq + q];
      if (c.pos_has_cls && s == 0) o = f4_add(o, pos[q]);
    } else if (s < c.n_tokens) {
      o = f4_add(y[(size_t)t * dq + q], pos[(size_t)(s - c.n_prefix + c.pos_has_cls) * dq + q]);
    }
    x[(size_t)t * dq + q] = o;
  }
}

// Backward of s3_embed_kernel.  dx [batch * s_pad, dim] (the gradient w.r.t. the first block's input) in, per token row s
// and float4 column q:  dprefix[s] += sum_b dx[b, s]  (s < n_prefix),  dpos[row of s] += sum_b dx[b, s]  (the cls row when
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
  S2_TRY(pos_pass<false>(pos + c, tmp, nullptr, nullptr, PosPass{wx, g0, gw, g0, 1, g0, 1, g0, 0, 1, dq}, s));
  // y pass: O[i, j] = sum_p Wy[i, p] T[p, j]
  return pos_pass<false>(tmp, out + c, has_cls ? pos : nullptr, out, PosPass{wy, gh, gw, g0, 0, g0, 1, 0, 1, gw, dq}, s);
}

// dout [has_cls + gh gw, dim] -> dpos [has_cls + g0 g0, dim] += its transpose; tmp [g0, gw, dim]
int pos_resample_bwd(const float* dout, float* dpos, const float* wy, const float* wx, float* tmp, int g0, int gh, int gw,
                     int dim, int has_cls, hipStream_t s) {
  const int dq = dim / 4, c = has_cls * dim;
  // dT[p, j] = sum_i Wy[i, p] dO[i, j]
  S2_TRY(pos_pass<false>(dout + c, tmp, nullptr, nullptr, PosPass{wy, g0, gw, gh, 0, 1, g0, 0, 1, gw, dq}, s));
  // dP[p, q] += sum_j Wx[j, q] dT[p, j]: a gather down the table's column q
  return pos_pass<true>(tmp, dpos + c, has_cls ? dout : nullptr, dpos, PosPass{wx, g0, g0, gw, 1, 1, g0, gw, 0, 1, dq}, s);
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


// ---- host side ------------------------------------------------------------------------------------------
enum { PATCHW = 0, PATCHB, CLS, REG, POS, BLK0 };
enum { N1W = 0, N1B, QKVW, QKVB, PROJW, PROJB, LS1, N2W, N2B, FC1W, FC1B, FC2W, FC2B, LS2 };

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

struct S3Block {  // activations a block keeps for its backward pass
  float *xin, *xn1, *mean1, *rstd1, *qkv, *P, *ao, *f1, *x1, *xn2, *mean2, *rstd2, *h, *a, *f2;
};
struct S3Work {
  S3Block blk[DVT_VIT_MAX_DEPTH];
  float *xl, *xf, *meanf, *rstdf;  // the last block's output and its final norm
  float *col, *wpad, *dwpad, *emb;
  float *d0, *d1, *d2, *dh, *dqkv, *dP, *acc, *wT, *rowdot;
  float *pos, *dpos, *ptmp;  // the run-grid position table, its gradient and the resample's [g0, gw, dim] intermediate
  // gemm_mode 1 only: per block the qkv / proj / fc1 / fc2 weights as bf16, as stored [n, k] (the forward's B operand) and
  // transposed [k, n] (the data gradient's), and one bf16 scratch for the A operand of the GEMM about to run
  uint16_t *wb[DVT_VIT_MAX_DEPTH][4], *wtb[DVT_VIT_MAX_DEPTH][4], *abf;
};

// the table's grid differs from the run's: the step resamples pos_embed on its way in and its gradient on the way out
bool resamples(const DvtVitConfig* c, int g0) { return g0 > 0 && (g0 != c->grid_h || g0 != c->grid_w); }

int64_t carve(const DvtVitConfig* c, int batch, char* base, S3Work* w, int g0 = 0, int mode = 0) {
  const int64_t R = (int64_t)batch * c->s_pad, C = c->dim, F = c->mlp_dim;
  const int64_t PP = (int64_t)batch * c->heads * c->s_pad * c->s_pad;
  int64_t o = 0;
  auto take = [&](int64_t floats) {
    float* p = base ? reinterpret_cast<float*>(base + o) : nullptr;
    o += (floats * 4 + 255) / 256 * 256;
    return p;
  };
  S3Work t{};
  for (int b = 0; b < c->depth; ++b) {
    S3Block& k = t.blk[b];
    k.xin = take(R * C);
    k.xn1 = take(R * C);
    k.mean1 = take(R);
    k.rstd1 = take(R);
    k.qkv = take(R * 3 * C);
    k.P = take(PP);
    k.ao = take(R * C);
    k.f1 = take(R * C);
    k.x1 = take(R * C);
    k.xn2 = take(R * C);
    k.mean2 = take(R);
    k.rstd2 = take(R);
    k.h = take(R * F);
    k.a = take(R * F);
    k.f2 = take(R * C);
  }
  t.xl = take(R * C);
  t.xf = take(R * C);
  t.meanf = take(R);
  t.rstdf = take(R);
  t.col = take(R * c->k_patch);
  t.wpad = take(C * c->k_patch);
  t.dwpad = take(C * c->k_patch);
  t.emb = take(R * C);
  t.d0 = take(R * C);
  t.d1 = take(R * C);
  t.d2 = take(R * C);
  t.dh = take(R * F);
  t.dqkv = take(R * 3 * C);
  t.dP = take(PP);
  t.acc = take(64);
  t.wT = take((3 * C > F ? 3 * C : F) * C);
  t.rowdot = take((int64_t)batch * c->heads * c->s_pad);
  if (resamples(c, g0)) {  // behind everything else: the equal-grid workspace is what it always was
    const int64_t n = (int64_t)(c->pos_has_cls + c->grid_h * c->grid_w) * C;
    t.pos = take(n);
    t.dpos = take(n);
    t.ptmp = take((int64_t)g0 * c->grid_w * C);
  }
  if (mode == 1) {  // behind everything else again: the fp32 mode's sizes and carving are what they were
    auto take16 = [&](int64_t halves) { return reinterpret_cast<uint16_t*>(take((halves + 1) / 2)); };
    const int64_t wn[4] = {3 * C * C, C * C, F * C, C * F};
    for (int b = 0; b < c->depth; ++b)
      for (int i = 0; i < 4; ++i) {
        t.wb[b][i] = take16(wn[i]);
        t.wtb[b][i] = take16(wn[i]);
      }
    t.abf = take16(R * (3 * C > F ? 3 * C : F));  // the widest A operand: a / dh [R, mlp_dim] or dqkv [R, 3 dim]
  }
  if (w) *w = t;
  return o;
}

int ls_add_ln(int C, const float* a, const float* f, const float* ls, float* sum_out, const float* g, const float* be,
              float* xn, float* mean, float* rstd, int T, int Tp, int R, float eps, hipStream_t s) {
  switch (C) {
    case 384: return launch_rows(s3_ls_add_ln_kernel<384>, R, s, a, f, ls, sum_out, g, be, xn, mean, rstd, T, Tp, R, eps);
    case 768: return launch_rows(s3_ls_add_ln_kernel<768>, R, s, a, f, ls, sum_out, g, be, xn, mean, rstd, T, Tp, R, eps);
    default: return launch_rows(s3_ls_add_ln_kernel<1024>, R, s, a, f, ls, sum_out, g, be, xn, mean, rstd, T, Tp, R, eps);
  }
}

int ls_bwd(int C, const float* dy, const float* f, const float* ls, float* df, float* dls, int R, hipStream_t s) {
  const dim3 grid(dvt_cdiv(R, 32)), blk(256);
  switch (C) {
    case 384: hipLaunchKernelGGL(s3_ls_bwd_kernel<384>, grid, blk, 0, s, dy, f, ls, df, dls, R); break;
    case 768: hipLaunchKernelGGL(s3_ls_bwd_kernel<768>, grid, blk, 0, s, dy, f, ls, df, dls, R); break;
    default: hipLaunchKernelGGL(s3_ls_bwd_kernel<1024>, grid, blk, 0, s, dy, f, ls, df, dls, R); break;
  }
  DVT_CHECK_LAUNCH();
  return 0;
}

// ---- gemm_mode 1: the forward and the data gradient of a linear layer on the extractor's bf16 GEMM (dvt_vit_gemm.hip, EPI_F32:
// bf16 operands, fp32 accumulation, fp32 output; m % 128 == n % 128 == k % 64 == 0, which check_cfg guarantees for every
// layer of the block: R = batch s_pad with s_pad % 128 == 0, dim in {384, 768, 1024}, mlp_dim % 128 == 0).  The A operand is
// rounded into `abf` right here; the weights were rounded at the top of run(). ----
bool mp_shape_ok(int R, int n, int k) { return R > 0 && R % 128 == 0 && n % 128 == 0 && k % 64 == 0; }

// y[R][n] = bf16(x)[R][k] . bf16(w)[n][k]^T + b
int lin_fwd_mp(const float* x, const uint16_t* wb, const float* b, float* y, int R, int n, int k, uint16_t* abf, hipStream_t s) {
  if (!mp_shape_ok(R, n, k)) return DVT_E_BADARG;
  S2_TRY(dvt_s3_cast_bf16(x, abf, R, k, s));
  return dvt_vit_gemm_f32out(abf, wb, b, y, R, n, k, s);
}

// dx[R][k] = bf16(dy)[R][n] . bf16(w^T)[k][n]^T;  dw[n][k] += dy^T . x and db[n] += colsum(dy) in exact fp32 from the UNROUNDED
// dy and x, on lin_bwd's side stream beside the data gradient as in the fp32 mode
int lin_bwd_mp(const float* dy, const float* x, const uint16_t* wtb, float* dx, float* dw, float* db, int R, int n, int k,
               uint16_t* abf, hipStream_t s) {
  if (!mp_shape_ok(R, k, n)) return DVT_E_BADARG;
  BlockFork f(s);
  S2_TRY(f.fork());
  S2_TRY(lin_bwd(dy, x, nullptr, nullptr, dw, db, R, n, k, f.side()));  // no dx: the weight and bias gradients alone, beside
  S2_TRY(dvt_s3_cast_bf16(dy, abf, R, n, s));
  S2_TRY(dvt_vit_gemm_f32out(abf, wtb, nullptr, dx, R, k, n, s));
  return f.join();
}

int run(const DvtVitConfig* c, const float* params, float* grads, const float* img, const float* target, float* feat,
        int batch, int norm_batch, void* work, int64_t work_bytes, float* loss_out, hipStream_t s, int g0 = 0,
        const float* wy = nullptr, const float* wx = nullptr, int mode = 0) {
  S2_TRY(check_cfg(c));
  if (mode != 0 && mode != 1) return DVT_E_BADARG;
  const bool rs = resamples(c, g0);
  if (rs) S2_TRY(pos_check(wy, wx, g0, c->grid_h, c->grid_w, c->dim, c->pos_has_cls));
  if (!params || !grads || !img || !target || !loss_out || !work || batch < 1 || norm_batch < batch) return DVT_E_BADARG;
  S3Work w;
  if (carve(c, batch, reinterpret_cast<char*>(work), &w, g0, mode) > work_bytes) return DVT_E_BADARG;
  if (mode == 1 && (!dvt_aligned16(params) || !dvt_aligned16(work))) return DVT_E_BADARG;  // (the casts move 16-byte pieces)
  int64_t po[8 + DVT_S3_TENSORS_PER_BLOCK * DVT_VIT_MAX_DEPTH];
  offsets(c, po, g0);
  const int C = c->dim, F = c->mlp_dim, T = c->n_tokens, Tp = c->s_pad, H = c->heads, NB = c->depth;
  const int K0 = 3 * c->patch * c->patch, KP = c->k_patch;
  const int R = batch * Tp;
  const float scale = 0.125f;  // head_dim^-0.5
  const AttnDims ad{batch, H, T, Tp, C};
  auto P = [&](int b, int i) { return params + po[BLK0 + DVT_S3_TENSORS_PER_BLOCK * b + i]; };
  auto G = [&](int b, int i) { return grads + po[BLK0 + DVT_S3_TENSORS_PER_BLOCK * b + i]; };
  const int64_t normw = po[BLK0 + DVT_S3_TENSORS_PER_BLOCK * NB], normb = po[BLK0 + DVT_S3_TENSORS_PER_BLOCK * NB + 1];
  const bool mp = mode == 1;
  enum { WQKV = 0, WPROJ, WFC1, WFC2 };
  // the four linear layers of a block in either mode (i: the layer's weight among the block's tensors, j: among its bf16 copies)
  auto fwd = [&](int b, int i, int j, const float* x, float* y, int n, int k) {
    return mp ? lin_fwd_mp(x, w.wb[b][j], P(b, i + 1), y, R, n, k, w.abf, s) : lin_fwd(x, P(b, i), P(b, i + 1), y, R, n, k, s);
  };
  auto bwd = [&](int b, int i, int j, const float* dy, const float* x, float* dx, int n, int k) {
    return mp ? lin_bwd_mp(dy, x, w.wtb[b][j], dx, G(b, i), G(b, i + 1), R, n, k, w.abf, s)
              : lin_bwd(dy, x, P(b, i), dx, G(b, i), G(b, i + 1), R, n, k, s, w.wT);
  };
  if (mp) {  // the weights of this call, rounded once: `params` changes between steps, and a slice is a step's unit
    const int wi[4] = {QKVW, PROJW, FC1W, FC2W}, wn[4] = {3 * C, C, F, C}, wk[4] = {C, C, C, F};
    for (int b = 0; b < NB; ++b)
      for (int j = 0; j < 4; ++j) {
        S2_TRY(dvt_s3_cast_bf16(P(b, wi[j]), w.wb[b][j], wn[j], wk[j], s));
        S2_TRY(dvt_s3_cast_bf16_t(P(b, wi[j]), w.wtb[b][j], wn[j], wk[j], s));
      }
  }

  // ---- forward: patch embedding, token assembly, block 0's norm1 ----
  {
    const int64_t n = (int64_t)C * KP;
    hipLaunchKernelGGL(s3_pad_kernel, dim3(dvt_cdiv(n, 256)), dim3(256), 0, s, params + po[PATCHW], w.wpad, C, K0, KP);
    DVT_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(s3_im2col_kernel, dim3(R), dim3(256), 0, s, img, w.col, *c);
  DVT_CHECK_LAUNCH();
  S2_TRY(lin_fwd(w.col, w.wpad, params + po[PATCHB], w.emb, R, C, KP, s));
  if (rs) S2_TRY(pos_resample_fwd(params + po[POS], w.pos, wy, wx, w.ptmp, g0, c->grid_h, c->grid_w, C, c->pos_has_cls, s));
  hipLaunchKernelGGL(s3_embed_kernel, dim3(R), dim3(256), 0, s, (const float4*)w.emb, (float4*)w.blk[0].xin,
                     (const float4*)(params + po[CLS]), (const float4*)(rs ? w.pos : params + po[POS]), *c);
  DVT_CHECK_LAUNCH();
  S2_TRY(ls_add_ln(C, w.blk[0].xin, nullptr, nullptr, nullptr, P(0, N1W), P(0, N1B), w.blk[0].xn1, w.blk[0].mean1,
                   w.blk[0].rstd1, T, Tp, R, c->ln_eps, s));
  // ---- the blocks ----
  for (int b = 0; b < NB; ++b) {
    const S3Block& k = w.blk[b];
    S2_TRY(fwd(b, QKVW, WQKV, k.xn1, k.qkv, 3 * C, C));
    S2_TRY(block_attn_fwd(ad, k.qkv, k.P, k.ao, scale, true, s));  // (s_pad % 128 == 0: always the attention-row kernel)
    S2_TRY(fwd(b, PROJW, WPROJ, k.ao, k.f1, C, C));
    S2_TRY(ls_add_ln(C, k.xin, k.f1, P(b, LS1), k.x1, P(b, N2W), P(b, N2B), k.xn2, k.mean2, k.rstd2, T, Tp, R, c->ln_eps, s));
    S2_TRY(fwd(b, FC1W, WFC1, k.xn2, k.h, F, C));
    S2_TRY(gelu_fwd(k.h, k.a, (int64_t)R * F / 4, s));
    S2_TRY(fwd(b, FC2W, WFC2, k.a, k.f2, C, F));
    if (b + 1 < NB) {
      const S3Block& n = w.blk[b + 1];
      S2_TRY(ls_add_ln(C, k.x1, k.f2, P(b, LS2), n.xin, P(b + 1, N1W), P(b + 1, N1B), n.xn1, n.mean1, n.rstd1, T, Tp, R,
                       c->ln_eps, s));
    } else {
      S2_TRY(ls_add_ln(C, k.x1, k.f2, P(b, LS2), w.xl, params + normw, params + normb, w.xf, w.meanf, w.rstdf, T, Tp, R,
                       c->ln_eps, s));
    }
  }

  // ---- loss over the patch rows ----
  S2_TRY(loss_rows(false, C,w.xf, nullptr, target, feat, w.d1, w.acc, c->n_prefix, T, Tp, R, norm_batch, loss_out, s));
  // final norm: d0 = d xl
  S2_TRY(ln_bwd(C, w.d1, w.xl, w.meanf, w.rstdf, params + normw, nullptr, w.d0, grads + normw, grads + normb, R, s));

  // ---- backward: d0 holds the gradient w.r.t. the current block's OUTPUT ----
  for (int b = NB - 1; b >= 0; --b) {
    const S3Block& k = w.blk[b];
    // mlp: out = x1 + ls2 (.) fc2(gelu(fc1(norm2(x1))))
    S2_TRY(ls_bwd(C, w.d0, k.f2, P(b, LS2), w.d1, G(b, LS2), R, s));  // d1 = d f2
    S2_TRY(bwd(b, FC2W, WFC2, w.d1, k.a, w.dh, C, F));
    S2_TRY(gelu_bwd(k.h, w.dh, (int64_t)R * F / 4, s));
    S2_TRY(bwd(b, FC1W, WFC1, w.dh, k.xn2, w.d2, F, C));
    S2_TRY(ln_bwd(C, w.d2, k.x1, k.mean2, k.rstd2, P(b, N2W), w.d0, w.d1, G(b, N2W), G(b, N2B), R, s));  // d1 = d x1
    // attention: x1 = xin + ls1 (.) proj(attn(norm1(xin)))
    S2_TRY(ls_bwd(C, w.d1, k.f1, P(b, LS1), w.d0, G(b, LS1), R, s));  // d0 = d f1
    S2_TRY(bwd(b, PROJW, WPROJ, w.d0, k.ao, w.d2, C, C));  // d2 = d ao
    // as the stage-2 step, always with dS from the attention-row kernel (bits 3 and 4 of dvt_tune_set(18, .) are stage 2's)
    S2_TRY(block_attn_bwd(ad, k.qkv, k.P, k.ao, w.d2, w.dqkv, w.dP, w.rowdot, scale, true, true, s));
    S2_TRY(bwd(b, QKVW, WQKV, w.dqkv, k.xn1, w.d2, 3 * C, C));
    S2_TRY(ln_bwd(C, w.d2, k.xin, k.mean1, k.rstd1, P(b, N1W), w.d1, w.d0, G(b, N1W), G(b, N1B), R, s));  // d0 = d xin
  }
  // ---- token assembly and patch embedding ----
  {
    if (rs) {  // the assembly's backward adds into a zeroed run-grid gradient; the transpose pass adds that into `grads`
      const hipError_t e = hipMemsetAsync(w.dpos, 0, sizeof(float) * (size_t)(c->pos_has_cls + c->grid_h * c->grid_w) * C, s);
      if (e != hipSuccess) return (int)e;
    }
    const int64_t n = (int64_t)T * (C / 4);
    hipLaunchKernelGGL(s3_embed_bwd_kernel, dim3(dvt_cdiv(n, 256)), dim3(256), 0, s, (float4*)w.d0, (float4*)(grads + po[CLS]),
                       (float4*)(rs ? w.dpos : grads + po[POS]), batch, *c);
    DVT_CHECK_LAUNCH();
    if (rs) S2_TRY(pos_resample_bwd(w.dpos, grads + po[POS], wy, wx, w.ptmp, g0, c->grid_h, c->grid_w, C, c->pos_has_cls, s));
  }
  {
    const hipError_t e = hipMemsetAsync(w.dwpad, 0, sizeof(float) * (size_t)C * KP, s);
    if (e != hipSuccess) return (int)e;
  }
  S2_TRY(lin_bwd(w.d0, w.col, w.wpad, nullptr, w.dwpad, grads + po[PATCHB], R, C, KP, s));
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
  S2_TRY(check_cfg(cfg));
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
  S2_TRY(pos_check(wy, wx, g0, grid_h, grid_w, dim, has_cls));
  if (!pos || !out || !tmp || !dvt_aligned16(pos) || !dvt_aligned16(out) || !dvt_aligned16(tmp)) return DVT_E_BADARG;
  return pos_resample_fwd(pos, out, wy, wx, tmp, g0, grid_h, grid_w, dim, has_cls, (hipStream_t)stream);
}

extern "C" int dvt_pos_resample_bwd(const float* dout, float* dpos, const float* wy, const float* wx, float* tmp, int g0,
                                    int grid_h, int grid_w, int dim, int has_cls, void* stream) {
  S2_TRY(pos_check(wy, wx, g0, grid_h, grid_w, dim, has_cls));
  if (!dout || !dpos || !tmp || !dvt_aligned16(dout) || !dvt_aligned16(dpos) || !dvt_aligned16(tmp)) return DVT_E_BADARG;
  return pos_resample_bwd(dout, dpos, wy, wx, tmp, g0, grid_h, grid_w, dim, has_cls, (hipStream_t)stream);
}

extern "C" int dvt_s3_param_offsets_pos(const DvtVitConfig* cfg, int g0, int64_t* out) {
  if (!out || g0 < 1) return DVT_E_BADARG;
  S2_TRY(check_cfg(cfg));
  offsets(cfg, out, g0);
  return 0;
}

extern "C" int64_t dvt_s3_workspace_bytes_pos(const DvtVitConfig* cfg, int batch, int g0) {
  if (check_cfg(cfg) != 0 || batch < 1 || g0 < 1) return -1;
  return carve(cfg, batch, nullptr, nullptr, g0);
}

extern "C" int64_t dvt_s3_workspace_bytes_mp(const DvtVitConfig* cfg, int batch, int g0, int gemm_mode) {
  if (check_cfg(cfg) != 0 || batch < 1 || g0 < 0 || (gemm_mode != 0 && gemm_mode != 1)) return -1;
  return carve(cfg, batch, nullptr, nullptr, g0, gemm_mode);
}

extern "C" int dvt_s3_train_slice_pos_mp(const DvtVitConfig* cfg, int g0, const float* wy, const float* wx, int gemm_mode,
                                         const float* params, float* grads, const float* img, const float* target,
                                         float* feat_out, int batch, int norm_batch, void* work, int64_t work_bytes,
                                         float* loss_out, void* stream) {
  if (g0 < 0 || (gemm_mode != 0 && gemm_mode != 1)) return DVT_E_BADARG;
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

extern "C" int dvt_parts_s3_embed(const float* y, float* x, const float* prefix, const float* pos, int batch, int dim, int n_prefix,
                                  int n_tokens, int s_pad, int pos_has_cls, void* stream) {
  DvtVitConfig c;
  S2_TRY(parts_cfg(&c, dim, n_prefix, n_tokens, s_pad, pos_has_cls));
  if (!y || !x || !pos || (n_prefix > 0 && !prefix) || batch < 1 || !dvt_aligned16(y) || !dvt_aligned16(x) || !dvt_aligned16(prefix) || !dvt_aligned16(pos))
    return DVT_E_BADARG;
  hipLaunchKernelGGL(s3_embed_kernel, dim3(batch * s_pad), dim3(256), 0, (hipStream_t)stream, (const float4*)y, (float4*)x,
                     (const float4*)prefix, (const float4*)pos, c);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int dvt_parts_s3_embed_bwd(float* dx, float* dprefix, float* dpos, int batch, int dim, int n_prefix, int n_tokens,
                                      int s_pad, int pos_has_cls, void* stream) {
  DvtVitConfig c;
  S2_TRY(parts_cfg(&c, dim, n_prefix, n_tokens, s_pad, pos_has_cls));
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
  hipLaunchKernelGGL(s3_im2col_kernel, dim3(batch * s_pad), dim3(256), 0, (hipStream_t)stream, img, col, c);
  DVT_CHECK_LAUNCH();
  return 0;
}
