// The stage-2 denoiser's bf16 inference forward for gfx950: the block kernels of the ViT extractor (dvt_vit.hip's block loop,
// dvt_vit_gemm.hip, dvt_vit_attn.hip) over the denoiser's own sequence.  C ABI in include/dvt_denoiser.h.
//
// Reference: dvt/models/online_denoiser.py:59-104 (Denoiser.forward): x = vit features (final-normed patch tokens, NHWC);
// x = x + pos_embed; x = blocks(x); no final norm.  The exact-fp32 forward of the trainer is dvt_s2_forward (dvt_stage2.hip).
//
// This unit: the denoiser's configuration and its check, the entry kernel, and the two forwards
//   dvt_denoiser_forward_bf16   features in  -> entry kernel (+ pos_embed) -> n blocks -> rows out
//   dvt_vit_forward_denoised    image in     -> the extractor up to its last block -> entry kernel (final LayerNorm of the
//                                               patch rows, + pos_embed) -> n blocks -> rows out
// The denoiser's sequence: grid_h * grid_w token rows per image, no prefix rows, padded to s_pad rows (a multiple of 32); the
// rows up to a whole 256-row tile behind the last image are phantom rows as in the extractor.  Pad and phantom rows enter as
// zeros, so the forward does not depend on what the workspace held.
#include "../../include/dvt_denoiser.h"
#include "dvt_ln_row.h"
#include "dvt_vit_dev.h"

namespace {

struct EntryArgs {
  const float* src;      // stand-alone: feats [batch, n_tok, dim]; fused: the extractor's residual stream [batch * vit_s_pad, dim]
  const float* norm_w;   // fused: the extractor's final LayerNorm
  const float* norm_b;
  const float* pos;      // [n_tok, dim] or NULL
  float* orig;           // fused: [batch, n_tok, dim] or NULL
  float* x;              // [T, dim] the denoiser's residual stream
  bf16_t* xb;            // FOLD: bf16(x) [T, dim]
  float2* stats;         // FOLD: (mean, rstd) [T]
  int T, real_rows;      // rows incl. phantom rows; batch * s_pad
  int s_pad, n_tok, dim;
  int vit_s_pad, vit_n_prefix;
  float vit_eps, eps;
};

// One wave per row of the denoiser's sequence (row = b * s_pad + p).  A token row (p < n_tok) is the caller's feature row, or
// (FUSED) the final LayerNorm of row b * vit_s_pad + vit_n_prefix + p of the extractor's residual stream -- ln_row_stats /
// ln_row_piece, the device functions of the final-norm launch, so `orig` gets the bits of dvt_vit_forward -- plus pos_embed[p].
// Pad rows and phantom rows are zeros.  FOLD: besides x, bf16(x) and the row's two-pass (mean, rstd), what
// ln_cast_stats_kernel (dvt_vit.hip) writes behind the extractor's patch embedding.  dim <= 1024: 4 float4 slots per lane.
template <bool FUSED, bool FOLD>
__global__ __launch_bounds__(256) void denoiser_entry_kernel(EntryArgs a) {
  constexpr int NV = 4;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.T) return;
  const int b = row / a.s_pad, p = row - b * a.s_pad;
  const bool live = row < a.real_rows && p < a.n_tok;
  const int nq = a.dim >> 2;
  float4 v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    const size_t tok = (size_t)b * a.n_tok + p;
    if (FUSED) {
      const float4* xr = reinterpret_cast<const float4*>(a.src + ((size_t)b * a.vit_s_pad + a.vit_n_prefix + p) * a.dim);
      float mean, rstd;
      ln_row_stats<NV>(xr, nq, a.dim, a.vit_eps, lane, v, mean, rstd);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int q = lane + 64 * i;
        if (q < nq) {
          v[i] = ln_row_piece(v[i], mean, rstd, reinterpret_cast<const float4*>(a.norm_w)[q],
                              reinterpret_cast<const float4*>(a.norm_b)[q]);
          if (a.orig != nullptr) reinterpret_cast<float4*>(a.orig + tok * a.dim)[q] = v[i];
        }
      }
    } else {
      const float4* xr = reinterpret_cast<const float4*>(a.src + tok * a.dim);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int q = lane + 64 * i;
        if (q < nq) v[i] = xr[q];
      }
    }
    if (a.pos != nullptr) {
      const float4* pr = reinterpret_cast<const float4*>(a.pos + (size_t)p * a.dim);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int q = lane + 64 * i;
        if (q < nq) {
          const float4 e = pr[q];
          v[i] = make_float4(v[i].x + e.x, v[i].y + e.y, v[i].z + e.z, v[i].w + e.w);
        }
      }
    }
  }
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int q = lane + 64 * i;
    if (q < nq) {
      reinterpret_cast<float4*>(a.x + (size_t)row * a.dim)[q] = v[i];
      if (FOLD) {
        sum += v[i].x + v[i].y + v[i].z + v[i].w;
        uint2 pk;
        pk.x = pack2(v[i].x, v[i].y);
        pk.y = pack2(v[i].z, v[i].w);
        reinterpret_cast<uint2*>(a.xb + (size_t)row * a.dim)[q] = pk;
      }
    }
  }
  if (FOLD) {
    const float mean = wave_sum(sum) / (float)a.dim;
    float var = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int q = lane + 64 * i;
      if (q < nq) {
        const float d0 = v[i].x - mean, d1 = v[i].y - mean, d2 = v[i].z - mean, d3 = v[i].w - mean;
        var += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
      }
    }
    const float rstd = rsqrtf(wave_sum(var) / (float)a.dim + a.eps);
    if (lane == 0) a.stats[row] = make_float2(mean, rstd);
  }
}

int launch_entry(const EntryArgs& a, bool fused, bool fold, hipStream_t s) {
  const dim3 grid(dvt_cdiv(a.T, 4)), block(256);
  if (fused) {
    if (fold) hipLaunchKernelGGL((denoiser_entry_kernel<true, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((denoiser_entry_kernel<true, false>), grid, block, 0, s, a);
  } else {
    if (fold) hipLaunchKernelGGL((denoiser_entry_kernel<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((denoiser_entry_kernel<false, false>), grid, block, 0, s, a);
  }
  DVT_CHECK_LAUNCH();
  return 0;
}

int check_den_cfg(const DvtDenoiserConfig* c) {
  if (!c || (c->dim != 384 && c->dim != 768 && c->dim != 1024)) return DVT_E_BADARG;
  if (c->heads * 64 != c->dim || c->mlp_dim != 4 * c->dim) return DVT_E_BADARG;
  if (c->n_blocks < 1 || c->n_blocks > DVT_DENOISER_MAX_BLOCKS) return DVT_E_BADARG;
  if (c->grid_h < 1 || c->grid_w < 1 || (int64_t)c->grid_h * c->grid_w > (1 << 20)) return DVT_E_BADARG;
  if (c->n_tokens != c->grid_h * c->grid_w || c->s_pad % 32 || c->s_pad < c->n_tokens) return DVT_E_BADARG;
  if ((c->enable_pe != 0 && c->enable_pe != 1) || !(c->ln_eps > 0.f)) return DVT_E_BADARG;
  return 0;
}

// every pointer the block loop will read; the folded weights all six or none
int check_den_weights(const DvtDenoiserConfig* c, const DvtDenoiserWeights* w) {
  if (!w || (c->enable_pe && !w->pos_embed)) return DVT_E_BADARG;
  for (int l = 0; l < c->n_blocks; ++l) {
    const DvtVitBlockWeights& b = w->blocks[l];
    if (!b.norm1_w || !b.norm1_b || !b.qkv_w || !b.qkv_b || !b.proj_w || !b.proj_b || !b.ls1 || !b.norm2_w || !b.norm2_b ||
        !b.fc1_w || !b.fc1_b || !b.fc2_w || !b.fc2_b || !b.ls2)
      return DVT_E_BADARG;
    const int n_fold = !!b.qkv_wf + !!b.qkv_cs + !!b.qkv_bf + !!b.fc1_wf + !!b.fc1_cs + !!b.fc1_bf;
    if (n_fold != 0 && n_fold != 6) return DVT_E_BADARG;
  }
  return 0;
}

// a batch whose row count (the GEMMs' M, the row kernels' grids) stays far inside int
int check_den_batch(const DvtDenoiserConfig* c, int batch) {
  return (batch <= 0 || (int64_t)batch * c->s_pad > (1 << 24)) ? DVT_E_BADARG : 0;
}

VitBlockGeom den_geom(const DvtDenoiserConfig* c, int batch) {
  VitBlockGeom g;
  g.batch = batch; g.s_pad = c->s_pad; g.n_valid = c->n_tokens; g.heads = c->heads; g.dim = c->dim; g.mlp_dim = c->mlp_dim;
  g.swiglu = 0; g.eps = c->ln_eps;
  return g;
}

// entry kernel -> blocks -> rows out, over a carved workspace whose x (and xb, stats) the entry kernel fills
int den_run(const DvtDenoiserConfig* c, const DvtDenoiserWeights* w, EntryArgs e, bool fused, const VitWork& k, float* out,
            int batch, hipStream_t s) {
  const VitBlockGeom g = den_geom(c, batch);
  const bool fold = vit_blocks_fold(g, w->blocks, c->n_blocks);
  e.pos = c->enable_pe ? w->pos_embed : nullptr;
  e.x = k.x; e.xb = k.xb; e.stats = k.stats;
  e.T = (batch * c->s_pad + 255) / 256 * 256; e.real_rows = batch * c->s_pad;
  e.s_pad = c->s_pad; e.n_tok = c->n_tokens; e.dim = c->dim; e.eps = c->ln_eps;
  int rc = launch_entry(e, fused, fold, s);
  if (rc) return rc;
  rc = vit_run_blocks(g, w->blocks, c->n_blocks, k, fold, nullptr, nullptr, s);
  if (rc) return rc;
  return vit_launch_rows_out(k.x, out, batch, c->s_pad, c->n_tokens, c->dim, s);
}

}  // namespace

extern "C" int dvt_denoiser_struct_sizes(int64_t* out) {
  if (!out) return DVT_E_BADARG;
  out[0] = sizeof(DvtDenoiserConfig);
  out[1] = sizeof(DvtDenoiserWeights);
  return 0;
}

extern "C" int dvt_denoiser_config(int dim, int n_blocks, int grid_h, int grid_w, int enable_pe, int row_pad,
                                   DvtDenoiserConfig* c) {
  if (!c || row_pad <= 0 || row_pad % 32 || grid_h < 1 || grid_w < 1 || (int64_t)grid_h * grid_w > (1 << 20)) return DVT_E_BADARG;
  c->dim = dim;
  c->heads = dim / 64;
  c->mlp_dim = 4 * dim;
  c->n_blocks = n_blocks;
  c->grid_h = grid_h;
  c->grid_w = grid_w;
  c->n_tokens = grid_h * grid_w;
  c->s_pad = (c->n_tokens + row_pad - 1) / row_pad * row_pad;
  c->enable_pe = enable_pe != 0;
  c->ln_eps = 1e-6f;
  return check_den_cfg(c);
}

extern "C" int64_t dvt_denoiser_workspace_bytes(const DvtDenoiserConfig* c, int batch) {
  if (check_den_cfg(c) || check_den_batch(c, batch)) return -1;
  return vit_carve_geom(c->s_pad, c->dim, c->mlp_dim, 0, batch, nullptr, nullptr);
}

extern "C" int dvt_denoiser_forward_bf16(const DvtDenoiserConfig* c, const DvtDenoiserWeights* w, const float* feats, float* out,
                                         int batch, void* workspace, void* stream) {
  int rc = check_den_cfg(c);
  if (rc) return rc;
  if ((rc = check_den_weights(c, w)) || (rc = check_den_batch(c, batch))) return rc;
  if (!feats || !out || !workspace) return DVT_E_BADARG;
  VitWork k;
  vit_carve_geom(c->s_pad, c->dim, c->mlp_dim, 0, batch, (char*)workspace, &k);
  EntryArgs e{};
  e.src = feats;
  return den_run(c, w, e, false, k, out, batch, (hipStream_t)stream);
}

// The fused workspace: the extractor's carve, then the denoiser's residual stream [T2, dim] fp32.  Every other buffer of the
// denoiser's carve lies over the extractor's buffer of the same name: T2 <= T, the same dim and mlp_dim, s_pad2 <= s_pad, so
// none is larger, and all are free once the extractor's last fc2 has run (its x is what the entry kernel still reads).
static int fused_check(const DvtVitConfig* vc, const DvtDenoiserConfig* dc, int batch) {
  int rc = vit_check_cfg(vc);
  if (rc) return rc;
  if ((rc = check_den_cfg(dc)) || (rc = check_den_batch(dc, batch))) return rc;
  if (vc->mlp_kind != DVT_VIT_MLP_GELU || vc->dim != dc->dim || vc->mlp_dim != dc->mlp_dim || vc->heads != dc->heads)
    return DVT_E_BADARG;
  if (vc->grid_h != dc->grid_h || vc->grid_w != dc->grid_w || dc->s_pad > vc->s_pad) return DVT_E_BADARG;
  return 0;
}

extern "C" int64_t dvt_vit_workspace_bytes_denoised(const DvtVitConfig* vc, const DvtDenoiserConfig* dc, int batch) {
  if (fused_check(vc, dc, batch)) return -1;
  const int64_t T2 = ((int64_t)batch * dc->s_pad + 255) / 256 * 256;
  return vit_carve_geom(vc->s_pad, vc->dim, vc->mlp_dim, vc->k_patch, batch, nullptr, nullptr) + up256b(T2 * dc->dim * 4);
}

extern "C" int dvt_vit_forward_denoised(const DvtVitConfig* vc, const DvtVitWeights* vw, const DvtDenoiserConfig* dc,
                                        const DvtDenoiserWeights* dw, const float* img, float* out, float* original_feats,
                                        float* cls, int batch, void* workspace, void* stream) {
  int rc = fused_check(vc, dc, batch);
  if (rc) return rc;
  if ((rc = check_den_weights(dc, dw))) return rc;
  if (!vw || !vw->norm_w || !vw->norm_b || !img || !out || !workspace) return DVT_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  VitWork vk;
  if ((rc = vit_forward_blocks(vc, vw, img, nullptr, batch, vc->depth, workspace, stream, &vk))) return rc;
  if (cls != nullptr && (rc = vit_launch_cls_norm(vk.x, vc, vw->norm_w, vw->norm_b, cls, batch, s))) return rc;
  VitWork dk = vk;
  dk.x = (float*)((char*)workspace + vit_carve_geom(vc->s_pad, vc->dim, vc->mlp_dim, vc->k_patch, batch, nullptr, nullptr));
  EntryArgs e{};
  e.src = vk.x; e.norm_w = vw->norm_w; e.norm_b = vw->norm_b; e.orig = original_feats;
  e.vit_s_pad = vc->s_pad; e.vit_n_prefix = vc->n_prefix; e.vit_eps = vc->ln_eps;
  return den_run(dc, dw, e, true, dk, out, batch, s);
}
