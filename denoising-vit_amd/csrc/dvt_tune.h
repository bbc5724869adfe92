// dvt_tune_set(key, value) (dvt_tune.hip): every unit that owns knobs defines them, keeps them to itself and decodes its own
// keys.  A decoder answers 0 (taken), DVT_E_BADARG (its own, refused) or DVT_TUNE_NOT_MINE, which never leaves the callers
// here.  dvt_tune_set asks the units in the order of this list and the first that knows the (key, value) pair answers.
#pragma once

constexpr int DVT_TUNE_NOT_MINE = 1;
constexpr int VIT_TUNE_NOT_MINE = DVT_TUNE_NOT_MINE;  // as the ViT extractor's units (and csrc/lab/) spell it

int gemm_f32_tune(int key, int value);       // dvt_gemm_f32.hip: key 0 (tile), key 5 (k-depth)
int gemm_f32_big_tune(int key, int value);   // dvt_gemm_f32_big.hip: key 4, values 10 / 11
int gemm_f32_glds_tune(int key, int value);  // dvt_gemm_f32_glds.hip: key 4, values 2 / 3 (ring depth) and every other value
                                             // (ring off / on for the fit) -- so the 128 x 128 unit is asked first
int fit_tune(int key, int value);            // dvt_fit.hip: keys 8 .. 12 (and 15 in the developer library)
int fit_fused_tune(int key, int value);      // dvt_fit_fused.hip: keys 6, 7, 13, 14, 16
// key 1, 2, 3, 18: one key each, the value is theirs to decode
int dvt_vit_tune(int gemm_variant);
// ... which asks the units of the ViT extractor in this order -- the forward (dvt_vit.hip), the fp32 extractor
// (dvt_vit_f32.hip), attention (dvt_vit_attn.hip), GEMM (dvt_vit_gemm.hip) -- in the same way.
int vit_forward_tune(int v);
int vit_f32_tune(int v);
int vit_attn_tune(int v);
int vit_gemm_tune(int v);
int dvt_grid_tune(int lds_level_max);
int dvt_adam_tune(int zero_all);
int dvt_s2_tune(int mask);
