// Frozen DINOv2 ViT forward for gfx950: bf16 operands on v_mfma_f32_16x16x32_bf16, fp32
// accumulation / residual stream / LayerNorm / softmax.  C ABI in include/dvt_vit.h.
//
// Reference: dvt/models/vit_wrapper.py:122-143 (get_intermediate_layers ->
// timm.VisionTransformer.forward_intermediates [timm 1.0.7, third party, not in the tree]),
// called from main_img_denoising.py:317-323 and :332-336.  Block structure restated in
// x += ls1 * proj(MHA(LN1(x))); x += ls2 * fc2(GELU(fc1(LN2(x)))).
//
// Data layout in HBM (one forward of `batch` images):
//   tokens of an image are padded from 1370 to s_pad = 1408 (multiple of 128) rows so that
//   no 128-row GEMM tile and no 64-key attention tile straddles two images; pad keys are
//   masked in the softmax, pad rows never reach the output.
//   x      fp32 [batch*s_pad, dim]        residual stream
//   xn     bf16 [batch*s_pad, dim]        LayerNorm output / attention output (GEMM A operand)
//   qk     bf16 [batch*s_pad, 2*dim]      q | k, head-major inside (timm qkv layout)
//   vt     bf16 [batch, heads, 64, s_pad] V TRANSPOSED per head: written by the qkv GEMM
//                                         epilogue so that P.V can read key-contiguous operands
//   hid    bf16 [batch*s_pad, mlp_dim]    GELU(fc1)
//   col    bf16 [batch*s_pad, k_patch]    im2col of the input image
//   xb, st_part, stats                    bf16(x), partial row sums and (mean, rstd): the LayerNorm folded into the GEMMs
//
// This unit: configuration and workspace (VitWork / vit_carve_geom), the forward (vit_forward_blocks: patch embedding + the
// block loop vit_run_blocks, which the denoiser's forwards of dvt_denoiser.hip run over their own sequence; vit_forward_run and
// the three dvt_vit_forward* entry points), dvt_vit_tune, and the small HBM-bound kernels around the GEMMs -- all launched by the product:
//   im2col_pairs_kernel<14 / 16 / 8>, im2col_kernel   patch embedding's A operand (pairs: even geometry; else generic)
//   ln_cast_stats_kernel<NV>, ln_stats_finalize_kernel  the folded LayerNorm's row statistics (default path)
//   layernorm_kernel<false, NV>                       LayerNorm as a kernel (dvt_tune_set(1, -60), unfolded shapes)
//   layernorm_kernel<true, NV>, tap_kernel<NORM, NV>  final norm / the taps of dvt_vit_forward_taps, one wave per row
//   swiglu_act_kernel                                 dvt_vit_swiglu_act only (the extractor fuses it into fc1)
// The GEMMs (dvt_vit_gemm.hip: launch_gemm<EPI>) and attention (dvt_vit_attn.hip) are reached through dvt_vit_dev.h; a block is
// qkv GEMM -> attention -> proj GEMM (+ residual) -> fc1 GEMM (GELU / SwiGLU) -> fc2 GEMM (+ residual).
#include "dvt_ln_row.h"
#include "dvt_vit_dev.h"

namespace {

// (mu, rstd) of every row from the P column-block partials written by the residual epilogue (fixed order: the
// result does not depend on scheduling)
__global__ __launch_bounds__(256) void ln_stats_finalize_kernel(const float2* __restrict__ part, int P, int M, float inv_n,
                                                                float eps, float2* __restrict__ stats) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  float s1 = 0.f, s2 = 0.f;
  for (int q = 0; q < P; ++q) {
    const float2 v = part[(size_t)q * M + m];
    s1 += v.x;
    s2 += v.y;
  }
  const float mu = s1 * inv_n;
  const float var = fmaxf(s2 * inv_n - mu * mu, 0.f);
  stats[m] = make_float2(mu, rsqrtf(var + eps));
}

// After the patch embedding (whose epilogue is not a residual epilogue): bf16(x) and exact two-pass (mu, rstd)
// NV: float4 register slots per lane that hold the row (4: dim <= 1024, the S / B / L models; 6: dim <= 1536, ViT-g)
template <int NV = 4>
__global__ __launch_bounds__(256) void ln_cast_stats_kernel(const float* __restrict__ x, bf16_t* __restrict__ xb,
                                                            float2* __restrict__ stats, int rows, int dim, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float4* xr = reinterpret_cast<const float4*>(x + (size_t)row * dim);
  const int nq = dim >> 2;
  float4 v[NV];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int q = lane + 64 * i;
    if (q < nq) {
      v[i] = xr[q];
      sum += v[i].x + v[i].y + v[i].z + v[i].w;
      uint2 pk;
      pk.x = pack2(v[i].x, v[i].y);
      pk.y = pack2(v[i].z, v[i].w);
      reinterpret_cast<uint2*>(xb + (size_t)row * dim)[q] = pk;
    }
  }
  const float mean = wave_sum(sum) / (float)dim;
  float var = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int q = lane + 64 * i;
    if (q < nq) {
      const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
      var += a * a + b * b + c * c + d * d;
    }
  }
  const float rstd = rsqrtf(wave_sum(var) / (float)dim + eps);
  if (lane == 0) stats[row] = make_float2(mean, rstd);
}

// silu(gate) * value on a full-width bf16 row [gates | values] (dvt_vit_swiglu_act): 8 hidden units per thread
__global__ __launch_bounds__(256) void swiglu_act_kernel(const uint4* __restrict__ h, uint4* __restrict__ hid, long long n8,
                                                         int hq) {
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n8; q += (long long)gridDim.x * 256) {
    const long long r = q / hq;
    const int c = (int)(q - r * hq);
    const uint4 gv = h[r * 2 * hq + c], vv = h[r * 2 * hq + hq + c];
    const unsigned gw[4] = {gv.x, gv.y, gv.z, gv.w}, vw[4] = {vv.x, vv.y, vv.z, vv.w};
    unsigned o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float g0 = __uint_as_float(gw[i] << 16), g1 = __uint_as_float(gw[i] & 0xffff0000u);
      const float v0 = __uint_as_float(vw[i] << 16), v1 = __uint_as_float(vw[i] & 0xffff0000u);
      o[i] = pack2(silu_log2(g0) * v0, silu_log2(g1) * v1);
    }
    hid[q] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// ======================================================================================
// im2col for the patch embedding (Conv2d 3 -> dim, kernel = patch, stride)
// ======================================================================================
__global__ __launch_bounds__(256) void im2col_kernel(const float* __restrict__ img,
                                                     bf16_t* __restrict__ col, DvtVitConfig c, int real_rows) {
  const int t = blockIdx.x;  // token row in [0, batch*s_pad), then the phantom rows up to a whole 256-row tile
  const int b = t / c.s_pad, s = t - b * c.s_pad;
  bf16_t* dst = col + (size_t)t * c.k_patch;
  const int pp = c.patch * c.patch;
  if (t >= real_rows || s < c.n_prefix || s >= c.n_tokens) {
    for (int k = threadIdx.x; k < c.k_patch; k += 256) dst[k] = 0;
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
    dst[k] = f2bf(v);
  }
}

// The common geometry (round 6): patch size a compile-time EVEN constant, stride and image width even -- a thread moves PAIRS
// (k, k + 1) of one patch row (8-byte aligned loads, 4-byte stores) and the k -> (channel, ky, kx) split divides by literals
// (with run-time divisors hipcc spends ~25 VALU instructions per division: the generic kernel ran at 2.3 TB/s of traffic).
template <int PATCH>
__global__ __launch_bounds__(256) void im2col_pairs_kernel(const float* __restrict__ img, bf16_t* __restrict__ col, DvtVitConfig c,
                                                           int real_rows) {
  static_assert(PATCH % 2 == 0, "pairs never straddle a patch row");
  constexpr int PP = PATCH * PATCH;
  const int t = blockIdx.x;
  const int b = t / c.s_pad, s = t - b * c.s_pad;
  uint32_t* dst = reinterpret_cast<uint32_t*>(col + (size_t)t * c.k_patch);
  const int npair = c.k_patch >> 1;
  if (t >= real_rows || s < c.n_prefix || s >= c.n_tokens) {
    for (int q = threadIdx.x; q < npair; q += 256) dst[q] = 0u;
    return;
  }
  const int py = (s - c.n_prefix) / c.grid_w, px = (s - c.n_prefix) - py * c.grid_w;
  const float* src = img + (size_t)b * 3 * c.img_h * c.img_w + (size_t)(py * c.stride) * c.img_w + px * c.stride;
  for (int q = threadIdx.x; q < npair; q += 256) {
    const int k = 2 * q;
    uint32_t w = 0u;
    if (k < 3 * PP) {
      const int ch = k / PP, rem = k - ch * PP, ky = rem / PATCH, kx = rem - ky * PATCH;
      const float2 v = *reinterpret_cast<const float2*>(src + ((size_t)ch * c.img_h + ky) * c.img_w + kx);
      w = pack2(v.x, v.y);
    }
    dst[q] = w;
  }
}

// ======================================================================================
// LayerNorm: fp32 row -> bf16 row (or fp32 output for the final norm), one wave per row
// ======================================================================================
// NV: float4 register slots per lane that hold the row (4: dim <= 1024; 6: dim <= 1536, ViT-g)
template <bool FINAL, int NV = 4>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x,
                                                        const float* __restrict__ w,
                                                        const float* __restrict__ b,
                                                        bf16_t* __restrict__ y_bf16,
                                                        float* __restrict__ y_f32, int rows,
                                                        int dim, float eps, int s_pad,
                                                        int n_tokens, int n_prefix) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  size_t in_row = row;
  if (FINAL) {  // output row = b*(n_tokens-n_prefix) + (s-n_prefix), input row = b*s_pad + s
    const int per = n_tokens - n_prefix;
    const int bb = row / per, s = row - bb * per + n_prefix;
    in_row = (size_t)bb * s_pad + s;
  }
  const float4* xr = reinterpret_cast<const float4*>(x + in_row * dim);
  const int nq = dim >> 2;
  float4 v[NV];
  float mean, rstd;
  ln_row_stats<NV>(xr, nq, dim, eps, lane, v, mean, rstd);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int q = lane + 64 * i;
    if (q < nq) {
      const float4 o = ln_row_piece(v[i], mean, rstd, reinterpret_cast<const float4*>(w)[q], reinterpret_cast<const float4*>(b)[q]);
      if (FINAL) {
        reinterpret_cast<float4*>(y_f32 + (size_t)row * dim)[q] = o;
      } else {
        uint2 pk;
        pk.x = pack2(o.x, o.y);
        pk.y = pack2(o.z, o.w);
        reinterpret_cast<uint2*>(y_bf16 + (size_t)row * dim)[q] = pk;
      }
    }
  }
}

// The tap of dvt_vit_forward*_taps: the residual rows of x [batch * s_pad, dim] after one block, prefix rows to `prefix`
// [batch, n_prefix, dim] (NULL: dropped), patch rows NHWC to `feat` [batch, n_tokens - n_prefix, dim]; one wave per token row,
// rows = batch * n_tokens (the pad rows behind n_tokens and the phantom rows are never addressed).  NORM: the final LayerNorm
// of layernorm_kernel<true> / layernorm_f32_kernel<true> (ln_row_stats / ln_row_piece); else the rows as they are.
template <bool NORM, int NV>
__global__ __launch_bounds__(256) void tap_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                  const float* __restrict__ b, float* __restrict__ feat,
                                                  float* __restrict__ prefix, int rows, int dim, float eps, int s_pad,
                                                  int n_tokens, int n_prefix) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int bb = row / n_tokens, s = row - bb * n_tokens;
  float* y;
  if (s < n_prefix) {
    if (prefix == nullptr) return;
    y = prefix + ((size_t)bb * n_prefix + s) * dim;
  } else {
    y = feat + ((size_t)bb * (n_tokens - n_prefix) + (s - n_prefix)) * dim;
  }
  const float4* xr = reinterpret_cast<const float4*>(x + ((size_t)bb * s_pad + s) * dim);
  const int nq = dim >> 2;
  if (NORM) {
    float4 v[NV];
    float mean, rstd;
    ln_row_stats<NV>(xr, nq, dim, eps, lane, v, mean, rstd);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int q = lane + 64 * i;
      if (q < nq)
        reinterpret_cast<float4*>(y)[q] =
            ln_row_piece(v[i], mean, rstd, reinterpret_cast<const float4*>(w)[q], reinterpret_cast<const float4*>(b)[q]);
    }
  } else {  // (slot by slot: a row parked in an array here is demoted to LDS / scratch by the compiler)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int q = lane + 64 * i;
      if (q < nq) reinterpret_cast<float4*>(y)[q] = xr[q];
    }
  }
}

// LayerNorm folded into the qkv / fc1 GEMMs and the proj / fc2 residual epilogues (ln_fold)
int g_vit_fuse_ln = 1;

}  // namespace

// (VitWork: dvt_vit_dev.h)
int64_t vit_carve_geom(int s_pad, int dim, int mlp_dim, int k_patch, int batch, char* base, VitWork* w) {
  // rows: whole 256-row GEMM tiles -- an odd batch (s_pad = 1408 = 5.5 tiles) gets 128 phantom rows, computed and
  // never read, so that every batch takes the same kernels (results must not depend on how views are batched)
  const int64_t T = ((int64_t)batch * s_pad + 255) / 256 * 256;
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    char* p = base ? base + o : nullptr;
    o += up256b(bytes);
    return p;
  };
  VitWork t;
  t.x = (float*)take(T * dim * 4);
  t.xn = (bf16_t*)take(T * dim * 2);
  // (+ 128 rows: where s_pad is not a multiple of 128 the attention kernel's last query block / key tile of the LAST image read
  // up to 127 rows past batch * s_pad -- never used: masked keys, unstored queries -- which T does not always cover)
  t.qk = (bf16_t*)take((T + 128) * 2 * dim * 2);
  // (the phantom rows store no V^T (GemmBArgs::vt_rows): `batch` images are what is written and read; the spare image keeps
  // the layout of the workspace as it was)
  t.vt = (bf16_t*)take(((int64_t)batch + 1) * s_pad * dim * 2);
  t.hid = (bf16_t*)take(T * mlp_dim * 2);  // (SwiGLU: the half-width silu(gate) * value is all the fc1 GEMM writes)
  t.col = (bf16_t*)take(T * k_patch * 2);  // (the denoiser's sequences have no patch embedding: k_patch 0, no bytes)
  t.xb = (bf16_t*)take(T * dim * 2);
  t.st_part = (float2*)take((int64_t)(dim / 64) * T * 8);
  t.stats = (float2*)take(T * 8);
  if (w) *w = t;
  return o;
}

namespace {

int64_t vit_carve(const DvtVitConfig* c, int batch, char* base, VitWork* w) {
  return vit_carve_geom(c->s_pad, c->dim, c->mlp_dim, c->k_patch, batch, base, w);
}

// the final LayerNorm (fp32 out, prefix / pad rows dropped): the 4-slot instantiation up to dim 1024, 6 slots above (ViT-g)
void launch_final_norm(const float* x, const float* w, const float* b, float* y, int rows, int dim, float eps, int s_pad,
                       int n_tokens, int n_prefix, hipStream_t s) {
  if (dim <= 1024)
    hipLaunchKernelGGL((layernorm_kernel<true, 4>), dim3(dvt_cdiv(rows, 4)), dim3(256), 0, s, x, w, b, (bf16_t*)nullptr, y, rows,
                       dim, eps, s_pad, n_tokens, n_prefix);
  else
    hipLaunchKernelGGL((layernorm_kernel<true, 6>), dim3(dvt_cdiv(rows, 4)), dim3(256), 0, s, x, w, b, (bf16_t*)nullptr, y, rows,
                       dim, eps, s_pad, n_tokens, n_prefix);
}

// im2col of `rows` token rows (rows >= real_rows = batch * s_pad: the phantom rows behind the last image are zero-filled).
// The pair kernel where the patch size is one of its instantiations (14: DINOv2; 16, 8: DINO / DeiT-III / AugReg) and the
// geometry is even, else the generic kernel.
void launch_im2col(const DvtVitConfig* c, const float* img, bf16_t* col, int rows, int real_rows, hipStream_t s) {
  const bool even = c->stride % 2 == 0 && c->img_w % 2 == 0 && c->k_patch % 2 == 0;
  if (even && c->patch == 14)
    hipLaunchKernelGGL(im2col_pairs_kernel<14>, dim3(rows), dim3(256), 0, s, img, col, *c, real_rows);
  else if (even && c->patch == 16)
    hipLaunchKernelGGL(im2col_pairs_kernel<16>, dim3(rows), dim3(256), 0, s, img, col, *c, real_rows);
  else if (even && c->patch == 8)
    hipLaunchKernelGGL(im2col_pairs_kernel<8>, dim3(rows), dim3(256), 0, s, img, col, *c, real_rows);
  else
    hipLaunchKernelGGL(im2col_kernel, dim3(rows), dim3(256), 0, s, img, col, *c, real_rows);
}

int check_vit_cfg(const DvtVitConfig* c) {
  if (!c || c->dim <= 0 || c->dim % 128 || c->dim > 1536 || c->heads * 64 != c->dim) return DVT_E_BADARG;
  if (c->depth < 1 || c->depth > DVT_VIT_MAX_DEPTH || c->mlp_dim <= 0 || c->mlp_dim % 128) return DVT_E_BADARG;
  if (c->mlp_kind != DVT_VIT_MLP_GELU && c->mlp_kind != DVT_VIT_MLP_SWIGLU) return DVT_E_BADARG;
  // token rows per image: a multiple of 32 (bf16 path; dvt_vit_config writes the next multiple of 128, the fp32 paths' need)
  if (c->s_pad % 32 || c->s_pad < c->n_tokens || c->k_patch % 64) return DVT_E_BADARG;
  if (c->n_prefix < 1 || c->n_prefix > 9 || (c->pos_has_cls != 0 && c->pos_has_cls != 1)) return DVT_E_BADARG;
  if (c->n_tokens != c->n_prefix + c->grid_h * c->grid_w) return DVT_E_BADARG;
  return 0;
}

}  // namespace

// The forward's share of dvt_tune_set(1, v)
int vit_forward_tune(int v) {
  if (v == -60 || v == -61) {  // LayerNorm kernels (-60) / folded into the GEMMs (-61, default)
    g_vit_fuse_ln = v == -61;
    return 0;
  }
  return VIT_TUNE_NOT_MINE;
}

// dvt_tune_set(1, v): every unit decodes the keys of its own knobs (dvt_vit_dev.h); the first that knows v answers.  The order
// matters in the developer build only, whose attention masks -540 - x and GEMM keys -600 - n / -700 - pct / -1100 - n share
// ranges (lab_attn_tune, lab/dvt_vit_lab_attn.inc); the product library's keys are disjoint.  Unknown to all: DVT_E_BADARG.
int dvt_vit_tune(int v) {
  for (int (*unit)(int) : {vit_forward_tune, vit_f32_tune, vit_attn_tune, vit_gemm_tune}) {
    const int rc = unit(v);
    if (rc != VIT_TUNE_NOT_MINE) return rc;
  }
  return DVT_E_BADARG;
}

// 1 when this library was built with -DDVT_LAB (the developer build of tools/build_lab.py), else 0
extern "C" int dvt_vit_is_lab_build(void) {
#ifdef DVT_LAB
  return 1;
#else
  return 0;
#endif
}

extern "C" int dvt_vit_struct_sizes(int64_t* out) {
  if (!out) return DVT_E_BADARG;
  out[0] = sizeof(DvtVitConfig);
  out[1] = sizeof(DvtVitBlockWeights);
  out[2] = sizeof(DvtVitWeights);
  return 0;
}

extern "C" int dvt_vit_config(int dim, int depth, int patch, int stride, int img_h, int img_w,
                              DvtVitConfig* c) {
  return dvt_vit_config_reg(dim, depth, patch, stride, img_h, img_w, 0, c);
}

extern "C" int dvt_vit_config_reg(int dim, int depth, int patch, int stride, int img_h, int img_w,
                                  int n_reg_tokens, DvtVitConfig* c) {
  return dvt_vit_config_ex(dim, depth, patch, stride, img_h, img_w, n_reg_tokens, DVT_VIT_MLP_GELU, c);
}

extern "C" int dvt_vit_config_ex(int dim, int depth, int patch, int stride, int img_h, int img_w, int n_reg_tokens,
                                 int mlp_kind, DvtVitConfig* c) {
  if (mlp_kind != DVT_VIT_MLP_GELU && mlp_kind != DVT_VIT_MLP_SWIGLU) return DVT_E_BADARG;
  if (!c || n_reg_tokens < 0 || n_reg_tokens > 8 || dim <= 0 || dim % 64 || patch <= 0 || stride <= 0 || img_h < patch || img_w < patch)
    return DVT_E_BADARG;
  c->dim = dim;
  c->depth = depth;
  c->heads = dim / 64;
  // SwiGLU: the hidden width of timm's SwiGLUPacked / DINOv2's SwiGLUFFNFused at mlp_ratio 4, (int(4 dim * 2 / 3) + 7) / 8 * 8
  c->mlp_dim = mlp_kind == DVT_VIT_MLP_SWIGLU ? (4 * dim * 2 / 3 + 7) / 8 * 8 : 4 * dim;
  c->mlp_kind = mlp_kind;
  c->patch = patch;
  c->stride = stride;
  c->img_h = img_h;
  c->img_w = img_w;
  c->grid_h = (img_h - patch) / stride + 1;  // vit_wrapper.py:84-88 dynamic_feat_size
  c->grid_w = (img_w - patch) / stride + 1;
  c->n_prefix = 1 + n_reg_tokens;
  c->pos_has_cls = n_reg_tokens == 0;  // timm: the reg4 DINOv2 models use no_embed_class=True
  c->n_tokens = c->n_prefix + c->grid_h * c->grid_w;
  c->s_pad = (c->n_tokens + 127) / 128 * 128;
  c->k_patch = (3 * patch * patch + 63) / 64 * 64;
  c->ln_eps = 1e-6f;
  return check_vit_cfg(c);
}

// The forward's im2col alone: col bf16 [batch * s_pad, k_patch]
extern "C" int dvt_vit_im2col(const DvtVitConfig* c, const float* img, void* col, int batch, void* stream) {
  const int rc = check_vit_cfg(c);
  if (rc) return rc;
  if (!img || !col || batch <= 0 || c->patch <= 0 || c->stride <= 0 || 3 * c->patch * c->patch > c->k_patch) return DVT_E_BADARG;
  if ((c->grid_h - 1) * c->stride + c->patch > c->img_h || (c->grid_w - 1) * c->stride + c->patch > c->img_w) return DVT_E_BADARG;
  launch_im2col(c, img, (bf16_t*)col, batch * c->s_pad, batch * c->s_pad, (hipStream_t)stream);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t dvt_vit_workspace_bytes(const DvtVitConfig* c, int batch) {
  if (check_vit_cfg(c) || batch <= 0) return -1;
  return vit_carve(c, batch, nullptr, nullptr);
}

// hid [m, n_hidden] (bf16) = silu(h[:, :n_hidden]) * h[:, n_hidden:] of a full-width h [m, 2 n_hidden] (bf16, the checkpoint's
// column order): the UNFUSED form of the SwiGLU fc1 epilogue (dvt_vit_gemm_bias + this), kept for the A/B of
// tools/bench_vitg.py; the extractor does not launch it
extern "C" int dvt_vit_swiglu_act(const void* h, void* hid, long long m, int n_hidden, void* stream) {
  if (!h || !hid || m < 0 || n_hidden <= 0 || n_hidden % 8) return DVT_E_BADARG;
  if (m == 0) return 0;
  const long long n8 = m * (n_hidden / 8);
  const int blocks = (int)((n8 + 255) / 256 < 256 * 32 ? (n8 + 255) / 256 : 256 * 32);
  hipLaunchKernelGGL(swiglu_act_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint4*)h, (uint4*)hid, n8,
                     n_hidden / 8);
  DVT_CHECK_LAUNCH();
  return 0;
}

// xb = bf16(x) and two-pass (mean, rstd) of every row: the kernel behind the patch embedding of the folded forward
extern "C" int dvt_vit_ln_cast_stats(const float* x, void* xb, void* stats, int rows, int dim, float eps, void* stream) {
  if (!x || !xb || !stats || rows < 0 || dim <= 0 || dim % 4 || dim > 1536) return DVT_E_BADARG;
  if (rows == 0) return 0;
  if (dim <= 1024)
    hipLaunchKernelGGL(ln_cast_stats_kernel<4>, dim3(dvt_cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, (bf16_t*)xb,
                       (float2*)stats, rows, dim, eps);
  else
    hipLaunchKernelGGL(ln_cast_stats_kernel<6>, dim3(dvt_cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, (bf16_t*)xb,
                       (float2*)stats, rows, dim, eps);
  DVT_CHECK_LAUNCH();
  return 0;
}

// (mean, rstd) of `rows` rows from their n_part column-block partials: behind every residual GEMM of the folded forward, and
// behind dvt_vit_gemm_residual_stats (dvt_vit_gemm.hip)
int launch_ln_stats_finalize(const float2* part, int n_part, int rows, float inv_n, float eps, float2* stats, hipStream_t s) {
  hipLaunchKernelGGL(ln_stats_finalize_kernel, dim3(dvt_cdiv(rows, 256)), dim3(256), 0, s, part, n_part, rows, inv_n, eps, stats);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int dvt_vit_layernorm(const float* x, const float* w, const float* b, void* y, int rows,
                                 int dim, float eps, void* stream) {
  if (!x || !w || !b || !y || rows < 0 || dim <= 0 || dim % 4 || dim > 1536) return DVT_E_BADARG;
  if (rows == 0) return 0;
  if (dim <= 1024)
    hipLaunchKernelGGL((layernorm_kernel<false, 4>), dim3(dvt_cdiv(rows, 4)), dim3(256), 0,
                       (hipStream_t)stream, x, w, b, (bf16_t*)y, (float*)nullptr, rows, dim, eps, 0, 0, 0);
  else
    hipLaunchKernelGGL((layernorm_kernel<false, 6>), dim3(dvt_cdiv(rows, 4)), dim3(256), 0,
                       (hipStream_t)stream, x, w, b, (bf16_t*)y, (float*)nullptr, rows, dim, eps, 0, 0, 0);
  DVT_CHECK_LAUNCH();
  return 0;
}

// Host-side check of a tap list (include/dvt_vit.h), shared by the three tapped forwards: pure arithmetic on the two host
// structs, before any device pointer is looked at.
int dvt_vit_check_taps(const DvtVitConfig* c, const DvtVitTaps* t) {
  if (!c || !t || t->n_taps < 1 || t->n_taps > DVT_VIT_MAX_TAPS) return DVT_E_BADARG;
  for (int i = 0; i < t->n_taps; ++i) {
    if (t->block[i] < 0 || t->block[i] >= c->depth || (i > 0 && t->block[i] <= t->block[i - 1])) return DVT_E_BADARG;
    if (!t->feat[i] || (t->prefix[i] && c->n_prefix <= 0)) return DVT_E_BADARG;
  }
  return 0;
}

// One tap: the token rows of x after a block -> feat (patch rows, NHWC) and prefix (NULL: dropped); 4 register slots up to
// dim 1024, 6 above, as launch_final_norm.
int dvt_vit_launch_tap(const float* x, const DvtVitConfig* c, const float* norm_w, const float* norm_b, float* feat,
                       float* prefix, int batch, int norm, hipStream_t s) {
  const int rows = batch * c->n_tokens;
  const dim3 grid(dvt_cdiv(rows, 4)), block(256);
#define DVT_TAP(NORM, NV)                                                                                                  \
  hipLaunchKernelGGL((tap_kernel<NORM, NV>), grid, block, 0, s, x, norm_w, norm_b, feat, prefix, rows, c->dim, c->ln_eps, \
                     c->s_pad, c->n_tokens, c->n_prefix)
  if (c->dim <= 1024) {
    if (norm) DVT_TAP(true, 4);
    else DVT_TAP(false, 4);
  } else {
    if (norm) DVT_TAP(true, 6);
    else DVT_TAP(false, 6);
  }
#undef DVT_TAP
  DVT_CHECK_LAUNCH();
  return 0;
}

// What the denoiser's forwards (dvt_denoiser.hip) launch of this unit's kernels.
int vit_check_cfg(const DvtVitConfig* c) { return check_vit_cfg(c); }

int vit_launch_cls_norm(const float* x, const DvtVitConfig* c, const float* norm_w, const float* norm_b, float* cls, int batch,
                        hipStream_t s) {
  launch_final_norm(x, norm_w, norm_b, cls, batch, c->dim, c->ln_eps, c->s_pad, 1, 0, s);
  DVT_CHECK_LAUNCH();
  return 0;
}

int vit_launch_rows_out(const float* x, float* out, int batch, int s_pad, int n_valid, int dim, hipStream_t s) {
  const int rows = batch * n_valid;
  hipLaunchKernelGGL((tap_kernel<false, 4>), dim3(dvt_cdiv(rows, 4)), dim3(256), 0, s, x, (const float*)nullptr,
                     (const float*)nullptr, out, (float*)nullptr, rows, dim, 0.f, s_pad, n_valid, 0);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t dvt_vit_taps_struct_size(void) { return (int64_t)sizeof(DvtVitTaps); }

// LayerNorm folded into the GEMMs (ln_fold): needs the folded weights, the 8-phase kernel on every GEMM of the
// block (whole 256-row / 256-column tiles) and is switched by dvt_vit_tune; otherwise the LayerNorm kernels run.
bool vit_blocks_fold(const VitBlockGeom& g, const DvtVitBlockWeights* blocks, int n) {
  const int T = (g.batch * g.s_pad + 255) / 256 * 256;
  bool fuse_ln = g_vit_fuse_ln && vit_gemm_sq_schedule() && T % 256 == 0 && g.dim % 256 == 0 && g.mlp_dim % 256 == 0 && n > 0;
  for (int l = 0; l < n; ++l) {
    const DvtVitBlockWeights& bw = blocks[l];
    fuse_ln = fuse_ln && bw.qkv_wf && bw.qkv_cs && bw.qkv_bf && bw.fc1_wf && bw.fc1_cs && bw.fc1_bf;
  }
  return fuse_ln;
}

// The block loop of every bf16 forward (the extractor's and the denoiser's): qkv GEMM -> attention -> proj GEMM (+ residual)
// -> fc1 GEMM (GELU / SwiGLU) -> fc2 GEMM (+ residual), n times over the carved workspace.
int vit_run_blocks(const VitBlockGeom& g, const DvtVitBlockWeights* blocks, int n_blocks, const VitWork& k, bool fuse_ln,
                   int (*after_block)(void* ctx, int l), void* ctx, hipStream_t s) {
  const int T = (g.batch * g.s_pad + 255) / 256 * 256, D = g.dim;  // incl. phantom rows (vit_carve_geom)
  // algorithmic GEMM rows: the real tokens, not the rows padded to a multiple of 128
  const double rows = (double)g.batch * g.n_valid;
  const bool swiglu = g.swiglu != 0;
  const int n_part = D / 64;
  auto finalize_stats = [&]() { return launch_ln_stats_finalize(k.st_part, n_part, T, 1.0f / (float)D, g.eps, k.stats, s); };
  const bool log2q = vit_attn_q_prescaled();
  for (int l = 0; l < n_blocks; ++l) {
    const DvtVitBlockWeights& bw = blocks[l];
    if (!fuse_ln) DVT_TRY(dvt_vit_layernorm(k.x, bw.norm1_w, bw.norm1_b, k.xn, T, D, g.eps, s));
    {
      GemmBArgs a{};
      a.A = fuse_ln ? k.xb : k.xn; a.W = (const bf16_t*)(fuse_ln ? bw.qkv_wf : bw.qkv_w); a.M = T; a.N = 3 * D; a.K = D;
      a.bias = fuse_ln ? bw.qkv_bf : bw.qkv_b; a.out = k.qk; a.vt = k.vt;
      if (fuse_ln) { a.ln_stats = k.stats; a.ln_cs = bw.qkv_cs; }
      a.dim = D; a.heads = g.heads; a.s_pad = g.s_pad; a.n_tokens = g.n_valid; a.vt_rows = g.batch * g.s_pad;
      a.work = 2.0 * rows * 3.0 * D * D;
      a.q_scale = log2q ? ATT_Q_PRESCALE : 0.f;
      DVT_TRY(launch_gemm<EPI_QKV>(a, s));
    }
    if (log2q) DVT_TRY(dvt_vit_attention_log2q(k.qk, k.vt, k.xn, g.batch, g.heads, g.s_pad, g.n_valid, s));
    else DVT_TRY(dvt_vit_attention(k.qk, k.vt, k.xn, g.batch, g.heads, g.s_pad, g.n_valid, s));
    {
      GemmBArgs a{};
      a.A = k.xn; a.W = (const bf16_t*)bw.proj_w; a.M = T; a.N = D; a.K = D;
      a.bias = bw.proj_b; a.x = k.x; a.gamma = bw.ls1;
      if (fuse_ln) { a.xb = k.xb; a.st_part = k.st_part; }
      a.work = 2.0 * rows * D * D;
      DVT_TRY(launch_gemm<EPI_RESID>(a, s));
    }
    if (fuse_ln) {
      DVT_TRY(finalize_stats());
    } else {
      DVT_TRY(dvt_vit_layernorm(k.x, bw.norm2_w, bw.norm2_b, k.xn, T, D, g.eps, s));
    }
    {
      GemmBArgs a{};
      a.A = fuse_ln ? k.xb : k.xn; a.W = (const bf16_t*)(fuse_ln ? bw.fc1_wf : bw.fc1_w); a.M = T; a.N = g.mlp_dim; a.K = D;
      a.bias = fuse_ln ? bw.fc1_bf : bw.fc1_b; a.out = k.hid;
      if (fuse_ln) { a.ln_stats = k.stats; a.ln_cs = bw.fc1_cs; }
      if (swiglu) {  // packed [2 mlp_dim, dim] weights -> the half-width silu(gate) * value
        a.N = 2 * g.mlp_dim;
        a.work = 2.0 * rows * 2.0 * g.mlp_dim * D;
        DVT_TRY(launch_gemm<EPI_SWIGLU>(a, s));
      } else {
        a.work = 2.0 * rows * (double)g.mlp_dim * D;
        DVT_TRY(launch_gemm<EPI_GELU>(a, s));
      }
    }
    {
      GemmBArgs a{};
      a.A = k.hid; a.W = (const bf16_t*)bw.fc2_w; a.M = T; a.N = D; a.K = g.mlp_dim;
      a.bias = bw.fc2_b; a.x = k.x; a.gamma = bw.ls2;
      if (fuse_ln && l + 1 < n_blocks) { a.xb = k.xb; a.st_part = k.st_part; }
      a.work = 2.0 * rows * (double)g.mlp_dim * D;
      DVT_TRY(launch_gemm<EPI_RESID>(a, s));
    }
    if (fuse_ln && l + 1 < n_blocks) DVT_TRY(finalize_stats());
    // (the fc2 epilogue of a tapped inner block has written xb and the partials too: x is stored before either, the same
    // bits with or without them)
    if (after_block) DVT_TRY(after_block(ctx, l));
  }
  return 0;
}

namespace {
struct TapCtx {
  const DvtVitConfig* c;
  const DvtVitWeights* w;
  const DvtVitTaps* taps;
  const float* x;
  int batch, tap;
  hipStream_t s;
};
int tap_after_block(void* ctx, int l) {
  TapCtx& t = *(TapCtx*)ctx;
  if (t.tap < t.taps->n_taps && l == t.taps->block[t.tap]) {
    DVT_TRY(dvt_vit_launch_tap(t.x, t.c, t.w->norm_w, t.w->norm_b, t.taps->feat[t.tap], t.taps->prefix[t.tap], t.batch,
                               t.taps->norm, t.s));
    ++t.tap;
  }
  return 0;
}
}  // namespace

// The extractor up to the end of block n_blocks - 1: patch embedding, then the block loop (with `taps`, one tap launch behind
// every tapped block).  What dvt_vit_forward, dvt_vit_forward_taps and dvt_vit_forward_denoised have in common.
int vit_forward_blocks(const DvtVitConfig* c, const DvtVitWeights* w, const float* img, const DvtVitTaps* taps, int batch,
                       int n_blocks, void* workspace, void* stream, VitWork* k_out) {
  int rc = check_vit_cfg(c);
  if (rc) return rc;
  if (!w || !img || !workspace || batch <= 0 || n_blocks < 0 || n_blocks > c->depth) return DVT_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  VitWork k;
  vit_carve(c, batch, (char*)workspace, &k);
  if (k_out) *k_out = k;
  const int T = (batch * c->s_pad + 255) / 256 * 256, D = c->dim;  // incl. phantom rows (vit_carve)

  // patch embedding: im2col -> GEMM with the (+bias, +pos_embed, cls) epilogue
  launch_im2col(c, img, k.col, T, batch * c->s_pad, s);
  DVT_CHECK_LAUNCH();
  {
    GemmBArgs a{};
    a.A = k.col; a.W = (const bf16_t*)w->patch_w; a.M = T; a.N = D; a.K = c->k_patch;
    a.bias = w->patch_b; a.x = k.x; a.pos = w->pos_embed; a.cls = w->cls_token;
    a.s_pad = c->s_pad; a.n_tokens = c->n_tokens; a.dim = D; a.heads = c->heads;
    a.n_prefix = c->n_prefix; a.pos_has_cls = c->pos_has_cls;
    a.work = 2.0 * (double)batch * c->grid_h * c->grid_w * D * (3.0 * c->patch * c->patch);
    DVT_TRY(launch_gemm<EPI_EMBED>(a, s));
  }
  VitBlockGeom g;
  g.batch = batch; g.s_pad = c->s_pad; g.n_valid = c->n_tokens; g.heads = c->heads; g.dim = D; g.mlp_dim = c->mlp_dim;
  g.swiglu = c->mlp_kind == DVT_VIT_MLP_SWIGLU; g.eps = c->ln_eps;
  const bool fuse_ln = vit_blocks_fold(g, w->blocks, n_blocks);
  if (fuse_ln) {
    DVT_TRY(dvt_vit_ln_cast_stats(k.x, k.xb, k.stats, T, D, c->ln_eps, s));
  }
  TapCtx tc{c, w, taps, k.x, batch, 0, s};
  return vit_run_blocks(g, w->blocks, n_blocks, k, fuse_ln, taps ? tap_after_block : nullptr, &tc, s);
}

// dvt_vit_forward (taps == NULL: n_blocks blocks, the final LayerNorm into feat) and dvt_vit_forward_taps (feat == NULL:
// the blocks up to the last tap, one tap launch behind every tapped block) are the same launches in the same order.
static int vit_forward_run(const DvtVitConfig* c, const DvtVitWeights* w, const float* img, float* feat,
                           const DvtVitTaps* taps, int batch, int n_blocks, void* workspace, void* stream) {
  if (!feat && !taps) return DVT_E_BADARG;
  VitWork k;
  DVT_TRY(vit_forward_blocks(c, w, img, taps, batch, n_blocks, workspace, stream, &k));
  if (taps) return 0;
  // final LayerNorm, drop cls/pad rows, NHWC fp32 straight into the feature store
  const int out_rows = batch * (c->n_tokens - c->n_prefix);
  launch_final_norm(k.x, w->norm_w, w->norm_b, feat, out_rows, c->dim, c->ln_eps, c->s_pad, c->n_tokens, c->n_prefix,
                    (hipStream_t)stream);
  DVT_CHECK_LAUNCH();
  return 0;
}

extern "C" int dvt_vit_forward(const DvtVitConfig* c, const DvtVitWeights* w, const float* img,
                               float* feat, int batch, int n_blocks, void* workspace,
                               void* stream) {
  return vit_forward_run(c, w, img, feat, nullptr, batch, n_blocks, workspace, stream);
}

extern "C" int dvt_vit_forward_taps(const DvtVitConfig* c, const DvtVitWeights* w, const float* img, const DvtVitTaps* taps,
                                    int batch, void* workspace, void* stream) {
  const int rc = dvt_vit_check_taps(c, taps);
  if (rc) return rc;
  return vit_forward_run(c, w, img, nullptr, taps, batch, taps->block[taps->n_taps - 1] + 1, workspace, stream);
}

// The forward plus the final-normed cls row of every image: cls [batch, dim] fp32.  The patch tokens are the plain
// forward's; the cls rows come from the same residual stream (row b * s_pad of the workspace) through the same kernel.
extern "C" int dvt_vit_forward_cls(const DvtVitConfig* c, const DvtVitWeights* w, const float* img, float* feat,
                                   float* cls, int batch, int n_blocks, void* workspace, void* stream) {
  if (!cls) return DVT_E_BADARG;
  const int rc = dvt_vit_forward(c, w, img, feat, batch, n_blocks, workspace, stream);
  if (rc) return rc;
  VitWork k;
  vit_carve(c, batch, (char*)workspace, &k);
  launch_final_norm(k.x, w->norm_w, w->norm_b, cls, batch, c->dim, c->ln_eps, c->s_pad, 1, 0, (hipStream_t)stream);
  DVT_CHECK_LAUNCH();
  return 0;
}
