/*
 * dvt_denoiser.h -- C ABI of the stage-2 denoiser's bf16 INFERENCE forward in libdvt_hip.so (gfx950).
 *
 * The reference's Denoiser (dvt/models/online_denoiser.py:13-104) is `num_blocks` timm Blocks (pre-norm, LayerNorm eps 1e-6,
 * exact GELU, head_dim 64, no LayerScale, no final norm) over the ViT's final-normed patch tokens plus its own pos_embed.
 * dvt_s2_forward (dvt_stage2.h) is that forward in exact fp32, the trainer's; the entry points here run it on the block
 * kernels of the bf16 extractor (dvt_vit.h: bf16 operands on the matrix pipe, fp32 accumulation, residual stream, LayerNorm
 * statistics, softmax and epilogues) -- the arithmetic of the reference's `--dtype bfloat16` autocast mode.  Opt-in: nothing
 * calls them unless asked (dvt_amd: Denoiser(inference_dtype="bfloat16")).
 *
 * The denoiser's sequence has no prefix tokens: an image is grid_h * grid_w token rows padded to s_pad rows (a multiple of
 * 32), pad keys masked in the softmax.  Same conventions as dvt_vit.h (int return codes, device pointers owned by the caller,
 * hipStream_t as void*).
 */
#ifndef DVT_DENOISER_H
#define DVT_DENOISER_H

#include <stdint.h>

#include "dvt_vit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DVT_DENOISER_MAX_BLOCKS 8 /* == dvt_amd.s2.MAX_BLOCKS */

typedef struct DvtDenoiserConfig {
  int32_t dim;            /* 384 / 768 / 1024 (what the stage-2 kernels are built for) */
  int32_t heads;          /* dim / 64 */
  int32_t mlp_dim;        /* 4 * dim (GELU MLP) */
  int32_t n_blocks;       /* 1 .. DVT_DENOISER_MAX_BLOCKS */
  int32_t grid_h, grid_w; /* the token grid of this call */
  int32_t n_tokens;       /* grid_h * grid_w: no prefix tokens */
  int32_t s_pad;          /* token rows per image: >= n_tokens, a multiple of 32 */
  int32_t enable_pe;      /* 1: pos_embed is added to the input rows */
  float ln_eps;           /* 1e-6 */
} DvtDenoiserConfig;

/* Matrices bf16 [out, in], vectors fp32, as DvtVitBlockWeights.  ls1 / ls2 are ones (the Block has no LayerScale); the folded
 * weights (all six of every block, or none) select the LayerNorm-folded GEMMs where dim % 256 == 0 (768, 1024), else and at
 * dim 384 the LayerNorm kernels run. */
typedef struct DvtDenoiserWeights {
  const float* pos_embed; /* [n_tokens, dim] fp32, already resampled to grid_h x grid_w; read only with enable_pe */
  DvtVitBlockWeights blocks[DVT_DENOISER_MAX_BLOCKS];
} DvtDenoiserWeights;

/* HOST: fill a config; row_pad (a positive multiple of 32) is what an image's rows are padded to.  DVT_E_BADARG for a dim
 * outside the list, n_blocks outside 1 .. DVT_DENOISER_MAX_BLOCKS, an empty grid. */
int dvt_denoiser_config(int dim, int n_blocks, int grid_h, int grid_w, int enable_pe, int row_pad, DvtDenoiserConfig* h_out);
int dvt_denoiser_struct_sizes(int64_t* h_out2); /* {DvtDenoiserConfig, DvtDenoiserWeights} */

/* feats [batch, grid_h * grid_w, dim] fp32 (the final-normed patch tokens) -> out, same shape: out = blocks(feats + pos_embed).
 * `workspace` (dvt_denoiser_workspace_bytes; -1 for bad arguments) needs no initialisation, as dvt_vit_forward's: pad rows and
 * the phantom rows up to a whole 256-row tile are zero-filled by the entry kernel.  Nothing is written behind `out`.
 * DVT_E_BADARG before any launch, nothing written: a NULL pointer (pos_embed only with enable_pe), a dim outside 384 / 768 /
 * 1024, heads != dim / 64, mlp_dim != 4 dim, n_tokens != grid_h * grid_w, s_pad % 32 != 0 or s_pad < n_tokens, n_blocks
 * outside 1 .. DVT_DENOISER_MAX_BLOCKS, batch <= 0, a block with a NULL weight, or with some but not all folded weights. */
int64_t dvt_denoiser_workspace_bytes(const DvtDenoiserConfig* h_cfg, int batch);
int dvt_denoiser_forward_bf16(const DvtDenoiserConfig* h_cfg, const DvtDenoiserWeights* h_w, const float* feats, float* out,
                              int batch, void* workspace, void* stream);

/* Image in, denoised features out of ONE launch sequence in one workspace: dvt_vit_forward's launches up to the end of block
 * depth - 1, then the denoiser's entry kernel reads the patch rows of the extractor's residual stream through the final
 * LayerNorm (the device function of the final-norm launch) instead of a feature tensor, then the denoiser's blocks.
 *   out            [batch, grid_h, grid_w, dim] fp32: the bits of dvt_denoiser_forward_bf16 on dvt_vit_forward's features
 *   original_feats NULL, or [batch, grid_h, grid_w, dim] fp32: the bits of dvt_vit_forward(n_blocks = depth)
 *   cls            NULL, or [batch, dim] fp32: the bits of dvt_vit_forward_cls
 * The denoiser's residual stream is a buffer of its own behind the extractor's workspace (the repack moves rows by n_prefix
 * and by s_pad - den.s_pad per image: in place, one workgroup would read rows another writes); its other buffers reuse the
 * extractor's, which are free by then.  dvt_vit_workspace_bytes keeps its values.
 * DVT_E_BADARG before any launch: whatever dvt_vit_forward or dvt_denoiser_forward_bf16 refuses, a denoiser whose dim or grid
 * is not the extractor's, den.s_pad > vit.s_pad, a SwiGLU extractor. */
int64_t dvt_vit_workspace_bytes_denoised(const DvtVitConfig* h_vit_cfg, const DvtDenoiserConfig* h_den_cfg, int batch);
int dvt_vit_forward_denoised(const DvtVitConfig* h_vit_cfg, const DvtVitWeights* h_vit_w, const DvtDenoiserConfig* h_den_cfg,
                             const DvtDenoiserWeights* h_den_w, const float* img, float* out, float* original_feats, float* cls,
                             int batch, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DVT_DENOISER_H */
