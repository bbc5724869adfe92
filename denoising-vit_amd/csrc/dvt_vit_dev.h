// dvt_vit_dev.h -- what more than one translation unit of the bf16 ViT extractor needs.  Internal (not part of the C ABI of
// include/dvt_vit.h); it defines no kernel.
//   dvt_vit_gemm.hip  the bf16 GEMM family (its epilogues: dvt_vit_epilogue.h), launch_gemm<EPI>, the dvt_vit_gemm_* entry points
//   dvt_vit_attn.hip  the attention kernels and the dvt_vit_attention* entry points
//   dvt_vit.hip       im2col / LayerNorm / tap kernels, configuration, workspace and the forward loop
//   dvt_denoiser.hip  the stage-2 denoiser's bf16 inference forwards: its entry kernel, then the same block loop
// Here: the vector typedefs and the fp32 -> bf16 pack, the GEMM's argument block and epilogue / cache-policy enums, the tile
// and query-block sizes the host code of several units computes grids and workspaces from, the bf16x3 scratch layout, and the
// declarations of the host functions that cross units (bottom).  A __global__ kernel is launched only from the unit that
// defines it: what crosses a unit is always a host launcher.  Every unit keeps its dvt_tune_set(1, v) knobs to itself.
#pragma once
#include <math.h>

#include "../../include/dvt_vit.h"
#include "dvt_common.h"
#include "dvt_tune.h"
// ---- tile order: blockIdx -> (m, n) tile, L2-aware (map_tile, map_tile_fast, map_tile_id, fd_make / fd_div); here because
// the GEMM's argument block carries a TileOrder --------------------------------------------------------------------------
#include "dvt_tile_map.h"

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short bf16_t;

// The argument block of one bf16 GEMM launch: what the forward loop and the entry points fill in, launch_gemm<EPI> completes
// (group, mblock, ord, the policies) and every GEMM kernel takes by value -- as GemmBArgs, below.
struct GemmArgs {
  const bf16_t* A;
  const bf16_t* W;
  int M, N, K;
  const float* bias;  // [N]
  bf16_t* out;        // EPI_BIAS / EPI_GELU: [M, N]; EPI_QKV: qk [M, 2*dim]; EPI_SWIGLU: [M, N / 2]
  bf16_t* vt;         // EPI_QKV: [batch, heads, 64, s_pad]
  bf16_t* out_lo;     // EPI_QKV_X3: the lo parts of q | k ...
  bf16_t* vt_lo;      // ... and of V^T
  float* x;           // EPI_RESID / EPI_EMBED: residual stream [M, N]; EPI_F32: the fp32 output [M, N]
  const float* gamma; // EPI_RESID: LayerScale [N]
  const float* pos;   // EPI_EMBED: pos_embed [n_tokens, N]
  const float* cls;   // EPI_EMBED: prefix tokens [n_prefix, N] (cls, then register tokens)
  int dim, heads, s_pad, n_tokens;
  int n_prefix, pos_has_cls;  // EPI_EMBED: prefix rows; pos_embed row 0 belongs to cls (else patches only)
  int group;          // N tiles per L2-resident group (set by launch_gemm)
  int mblock;         // M panels per block of the tile order (1: n fastest)
  int nt_store;       // bf16 outputs with the non-temporal hint
  // LayerNorm folded into the GEMMs (see ln_fold): consumer side (EPI_QKV / EPI_GELU) ...
  const float2* ln_stats;  // [M] (mean, rstd) of the fp32 residual rows; A is then bf16(x), W is bf16(gamma (.) W)
  const float* ln_cs;      // [N] column sums of the folded weights
  // ... producer side (EPI_RESID): besides x, emit bf16(x) and the per-row partial sums of this 64-column block
  bf16_t* xb;              // [M, N]
  float2* st_part;         // [N / 64][M] (sum, sum of squares)
  float q_scale;      // EPI_QKV: the q columns (n < dim) leave multiplied by this (log2(e) / 8 for the log2-domain attention
                      // kernel); 0 = as they are
  int vt_rows;        // EPI_QKV / EPI_QKV_X3: batch * s_pad, the real token rows.  The phantom rows behind them (up to the
                      // whole 256-row tile) store their q | k but no V^T: `vt` holds `batch` images (their image index would
                      // run past it -- by up to 7 images at s_pad = 32)
  int dim_ok_sq;      // 256-wide tiles may be used (no q|k|v boundary inside a tile)
  int lda, ldw;       // leading dimensions (elements) of A and W; 0 = K
  double work;        // profiling probe: ALGORITHMIC flops of this launch (0: 2*M*N*K of the padded shape)
  unsigned* dbg;      // timing builds of the 8p kernel (dvt_vit_debug_buffer): 24 u32 per wave group and workgroup
  int stagger_ticks;  // 8p: the first round of workgroups (one per CU) starts spread over this many 100-MHz ticks (0: together)
  int tpw;            // lab 8t: tiles per workgroup (generations of 256 workgroups walk tpw x 256 consecutive tiles)
  // map_tile_fast: the 8p kernel's tile order (XCD column sets, groups, blocks and their divisors as multiply-shift pairs;
  // dvt_tile_map.h), set by launch_gemm for the 256 x 256 kernels.  ONLY gemm_bf16_kernel_8p reads it.  `group` / `mblock`
  // above are what every other kernel (pp, 128 x 128, the lab kernels) walks, always as ONE column set: with xcols > 1
  // ord.group is the column set's width (nt / xcols) and differs from `group` -- never mix the two in one kernel
  TileOrder ord;
  int pf_next;       // 8p: late in its epilogue a workgroup touches the first pf_next (0..2) k-tiles' operand lines of tile
                      // blockIdx + 256, the tile the next workgroup of its XCD walks (NextTilePf; dvt_tune_set(1, -570 - n))
  int abl;            // developer library, TIMING ONLY (dvt_tune_set(1, -560 - mask)): bit 0 = the epilogues do not park their
                      // accumulators in LDS (outputs are garbage): what the parking writes cost a tile
};

namespace {

typedef __bf16 hw_bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// fp32 -> bf16, round-to-nearest-even, through the gfx950 conversion instruction
// (v_cvt_pk_bf16_f32: one instruction per pair)
__device__ __forceinline__ uint32_t pack2(float a, float b) {
  const hw_bf16x2 v = __builtin_convertvector((f32x2){a, b}, hw_bf16x2);
  return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ bf16_t f2bf(float f) { return (bf16_t)(pack2(f, 0.f) & 0xffffu); }

// silu(g) = g * sigmoid(g) = g / (1 + 2^(-g log2 e)), the exponential in the log2 domain as in the attention kernel (one
// v_exp_f32).  The exponent is clamped at 126 so that 1 + 2^t stays finite: g = -100 gives -100 * 2^-126 (the true value,
// -3.7e-42, is below every output format's resolution) instead of -100 / inf; g -> +large gives g / 1.  No inf, no NaN for
// any finite g.  v_rcp_f32 is 1 ulp: far below the bf16 store.
__device__ __forceinline__ float silu_log2(float g) {
  const float e = __builtin_amdgcn_exp2f(fminf(g * -1.4426950408889634f, 126.f));
  return g * __builtin_amdgcn_rcpf(1.f + e);
}

// GEMM  C[M,N] = A[M,K] . W[N,K]^T: the 128 x 128 x 64 tile every shape check is written in (the 256-row / 256-column kernels
// take whole pairs of them)
constexpr int GBM = 128, GBN = 128, GBK = 64;

// EPI_F32: y = acc + bias written as fp32 into `x` (the bf16x3 GEMMs of the fp32 extractor, dvt_vit_f32.hip)
// EPI_GELU_X3 / EPI_QKV_X3 (same mode): the outputs leave as (hi, lo) bf16 splits of the fp32 values -- GELU(h) as the
// next GEMM's [hi | hi | lo] row (`out`, row stride 3 N), q | k as two [M, 2 dim] arrays (`out`, `out_lo`) and V^T as two
// [batch, heads, 64, s_pad] arrays (`vt`, `vt_lo`): what the split kernels + the qkv prep kernels would write.
// EPI_SWIGLU (ViT-g/14): W's rows arrive PACKED (dvt_vit_swiglu_pack_index) -- of a wave's 64 accumulator columns the first 32
// are gates, the last 32 the values of the same 32 hidden units -- and `out` is the half-width [M, N / 2] silu(gate) * value.
enum { EPI_BIAS = 0, EPI_QKV = 1, EPI_GELU = 2, EPI_RESID = 3, EPI_EMBED = 4, EPI_F32 = 5, EPI_GELU_X3 = 6, EPI_QKV_X3 = 7,
       EPI_SWIGLU = 8 };
#define IS_QKV(E) ((E) == EPI_QKV || (E) == EPI_QKV_X3)
#define IS_GELU(E) ((E) == EPI_GELU || (E) == EPI_GELU_X3)
#define IS_X3(E) ((E) == EPI_GELU_X3 || (E) == EPI_QKV_X3)

// Streaming (nt) cache policy for epilogue traffic that is touched once per launch (g_vit_epi_policy; dvt_tune_set(1,
// -200000 - mask)).  Policy only: no bit changes a result.
enum { EPOL_RESID_LD = 1,   // the fp32 residual loads of the 256 x 256 residual epilogue
       EPOL_RESID_ST = 2,   // ... its fp32 residual stores
       EPOL_XB_ST = 4,      // ... its bf16 xb stores (the next GEMM reads them, but only after 1.1 GB more has passed)
       EPOL_HID_ST = 8,     // the bf16 `out` stores of the bias / GELU / SwiGLU epilogues (hid)
       EPOL_QKV_ST = 16,    // the qk and V^T stores of the qkv epilogue
       EPOL_HID_SC1 = 32,   // the EPOL_HID_ST stores go out write-through (sc1: the line leaves the XCD's L2) instead of nt
       EPOL_RESID_SC1 = 64, // ... the EPOL_RESID_ST stores
       EPOL_ALL = 127,
       // shipped (profiles/r07/README.md): the residual stream nt on all three of its paths, hid write-through
       EPOL_DEFAULT = EPOL_RESID_LD | EPOL_RESID_ST | EPOL_XB_ST | EPOL_HID_ST | EPOL_HID_SC1 };

// The kernels' parameter type.  It stays a type of the anonymous namespace, so that every kernel keeps the name the committed
// profiles record (`gemm_bf16_kernel_8p<3, false, 0, 7>((anonymous namespace)::GemmBArgs)`); GemmArgs, the same bytes with
// external linkage, is what launch_gemm<EPI> takes across units.
struct GemmBArgs : GemmArgs {};

constexpr int ATT_Q = 128;  // queries per workgroup
constexpr float ATT_Q_PRESCALE = 0.125f * 1.4426950408889634f;

inline int64_t up256b(int64_t x) { return (x + 255) / 256 * 256; }

// scratch of the bf16x3 attention (elements of bf16): q|k hi [m, 2 dim], q|k lo [m, 2 dim], V^T hi and lo
// [batch + 1, heads, 64, s_pad] each; m = batch * s_pad rounded up to whole 256-row GEMM tiles (the fused qkv epilogue
// writes the q | k of those phantom rows but no V^T: images 0 .. batch - 1 of V^T hi / lo are written, image `batch` never)
struct X3Scratch {
  long long m, ql, vh, vl, total;
};
inline X3Scratch x3_scratch(int batch, int heads, int s_pad) {
  X3Scratch r;
  const long long dim = (long long)heads * 64;
  r.m = ((long long)batch * s_pad + 255) / 256 * 256;
  r.ql = r.m * 2 * dim;
  r.vh = 2 * r.ql;
  r.vl = r.vh + (long long)(batch + 1) * s_pad * dim;
  r.total = r.vl + (long long)(batch + 1) * s_pad * dim;
  return r;
}

}  // namespace

// ---- host functions that cross units (C++ linkage) ---------------------------------------------------------------------
// dvt_vit_gemm.hip: one GEMM launch; instantiated there for the nine epilogues.  DVT_E_BADARG for a shape or a combination of
// outputs that no kernel takes.
template <int EPI>
int launch_gemm(const GemmArgs& a, hipStream_t s);
// ... whether the selected schedule puts whole 256 x 256 tiles on the 8-phase kernel (what the folded LayerNorm needs)
bool vit_gemm_sq_schedule();
// dvt_vit_attn.hip: whether the forward's qkv GEMM is to write q pre-scaled by ATT_Q_PRESCALE and dvt_vit_attention_log2q to
// follow it (else q as it is and dvt_vit_attention)
bool vit_attn_q_prescaled();
// dvt_vit.hip: (mean, rstd) [rows] from the residual epilogues' partial sums part [n_part][rows] (ln_stats_finalize_kernel)
int launch_ln_stats_finalize(const float2* part, int n_part, int rows, float inv_n, float eps, float2* stats, hipStream_t s);
// dvt_vit.hip: the workspace of one forward and the block loop, shared with the denoiser's forwards (dvt_denoiser.hip)
struct VitWork {
  float* x;
  bf16_t *xn, *qk, *vt, *hid, *col;
  bf16_t* xb;       // bf16(x) for the LayerNorm-folded GEMMs
  float2* st_part;  // [dim / 64][T] partial row sums from the residual epilogues
  float2* stats;    // [T] (mean, rstd)
};
// what the block loop needs of a sequence: `batch` images of s_pad token rows each, the first n_valid of them tokens (the keys
// the attention sees); T = batch * s_pad rounded up to whole 256-row tiles
struct VitBlockGeom {
  int batch, s_pad, n_valid, heads, dim, mlp_dim, swiglu;
  float eps;
};
// ... the carve of `batch` images of s_pad rows (base == nullptr: the byte count alone; k_patch == 0: no im2col buffer)
int64_t vit_carve_geom(int s_pad, int dim, int mlp_dim, int k_patch, int batch, char* base, VitWork* w);
// ... whether n blocks at this geometry run with the LayerNorm folded into their GEMMs (the knob, the schedule, whole 256-wide
// tiles, and the folded weights of every block)
bool vit_blocks_fold(const VitBlockGeom& g, const DvtVitBlockWeights* blocks, int n);
// ... blocks[0 .. n - 1] over the carved workspace k (x, and with fuse_ln also xb and stats, hold the sequence); after block l
// after_block(ctx, l) runs where it is not NULL (the taps).  Launches only: the arguments are the caller's to check.
int vit_run_blocks(const VitBlockGeom& g, const DvtVitBlockWeights* blocks, int n, const VitWork& k, bool fuse_ln,
                   int (*after_block)(void* ctx, int l), void* ctx, hipStream_t s);
// ... the extractor up to the end of its blocks (everything of dvt_vit_forward but the final LayerNorm); *k: its carve
int vit_forward_blocks(const DvtVitConfig* c, const DvtVitWeights* w, const float* img, const DvtVitTaps* taps, int batch,
                       int n_blocks, void* workspace, void* stream, VitWork* k);
// ... the extractor's configuration check, and the final LayerNorm of the cls row of every image: cls [batch, dim] fp32 (the
// launch of dvt_vit_forward_cls)
int vit_check_cfg(const DvtVitConfig* c);
int vit_launch_cls_norm(const float* x, const DvtVitConfig* c, const float* norm_w, const float* norm_b, float* cls, int batch,
                        hipStream_t s);
// ... the first n_valid rows of every image of x [batch * s_pad, dim] as they are -> out [batch, n_valid, dim] fp32: the tap
// kernel without norm and without prefix rows (dim <= 1024)
int vit_launch_rows_out(const float* x, float* out, int batch, int s_pad, int n_valid, int dim, hipStream_t s);
// (the units' shares of dvt_tune_set(1, v) -- vit_forward_tune, vit_attn_tune, vit_gemm_tune and the fp32 extractor's
// vit_f32_tune -- are declared next to dvt_vit_tune in dvt_tune.h: dvt_vit_f32.hip does not include this header)
