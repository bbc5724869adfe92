// The trained transformer block of the stage-2 step (dvt_stage2.hip) and of the stage-3 step (dvt_stage3.hip), compiled once
// in dvt_block_train.hip: its pieces (linear layers, LayerNorm with the residual add in front and its backward, LayerScale
// backward, GELU, attention, loss rows, the side stream), the block's forward and backward launch sequences block_fwd /
// block_bwd at the end of this header, and the carving of a block's workspace.  Both steps keep what surrounds the blocks: input
// assembly, the norm behind each block, loss and optimizer.  Ordinary C++ functions, not part of the C ABI.
#pragma once
#include "dvt_common.h"

// dvt_stage2.hip: the process's A/B switches (dvt_tune_set(18, mask), DVT_S2_* in the environment) and the two softmax
// passes over a [rows][Tp] score matrix that the unfused attention branches run
extern int g_s2_fork_wgrad, g_s2_attn_rows, g_s2_fuse_softmax_bwd, g_s2_big_wgrad, g_s2_big_bwd, g_s2_big_fwd;
void s2_read_env();
int s2_softmax(float* S, int T, int Tp, int64_t rows, float scale, hipStream_t s);
int s2_softmax_bwd(const float* P, float* dP, int Tp, int64_t rows, float scale, hipStream_t s);

inline bool parts_c_ok(int C) { return C == 384 || C == 768 || C == 1024; }  // the widths the row kernels are built for

// One use, from the caller's stream s, of the side stream: one stream and two events per device, created together under a
// lock at the first use on that device and never destroyed.  fork(): the side stream waits for everything on s so far;
// join(): s waits for everything on the side stream so far; the destructor joins a fork left open, so an early return leaves
// nothing running beside the caller.  Both return 0 or the hipError_t.  Without a side stream (g_s2_fork_wgrad is 0, `want` is
// false, or one of the three creations failed) side() is s itself and fork() / join() do nothing.  The objects are shared by
// all callers on a device: the library supports one trainer per device and host thread at a time.
class BlockFork {
 public:
  explicit BlockFork(hipStream_t s, bool want = true);
  ~BlockFork() { join(); }
  BlockFork(const BlockFork&) = delete;
  hipStream_t side() const;
  int fork();
  int join();

 private:
  hipStream_t s_;
  const struct SideStream* side_;
  bool open_ = false;  // forked and not joined yet
};

// y[R][n] = x[R][k] . w[n][k]^T + b
int lin_fwd(const float* x, const float* w, const float* b, float* y, int R, int n, int k, hipStream_t s);
// dx[R][k] = dy[R][n] . w[n][k] (dx may be null);  dw[n][k] += dy^T . x;  db[n] += colsum(dy);  wT: scratch [k][n] or null
int lin_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* db, int R, int n, int k, hipStream_t s,
            float* wT = nullptr);
int ln_bwd(int C, const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* dres,
           float* dx, float* dgamma, float* dbeta, int R, hipStream_t s);
// a = gelu(h);  da *= gelu'(h) in place.  n4 float4 elements
int gelu_fwd(const float* h, float* a, int64_t n4, hipStream_t s);
int gelu_bwd(const float* h, float* da, int64_t n4, hipStream_t s);
// Clears acc, then dout and loss_out of `norm_batch` images' worth of loss rows (R rows are here); add: o = a + b, else o = a
int loss_rows(bool add, int C, const float* a, const float* b, const float* target, float* out, float* dout, float* acc,
              int n_prefix, int T, int Tp, int R, int norm_batch, float* loss_out, hipStream_t s);

// stage 3's gemm_modes 5 / 7 (dvt_s3_wgrad.hip): dw[n][k] (+)= bf16(dy)^T . bf16(x) from the row casts dyb [R][n], xb [R][k] that the
// caller made, db[n] (+)= colsum of the fp32 dy; S = dvt_s3_wgrad_splits(R, n, k) or a forced count in 1 .. R / 64; `partial` holds
// dvt_s3_wgrad_partial_bytes(R, n, k, S) bytes.  R, n, k multiples of 128, everything 16-byte aligned (the caller checks)
int dvt_s3_wgrad_splits(int64_t R, int n, int k);
int64_t dvt_s3_wgrad_partial_bytes(int64_t R, int n, int k, int S);
int dvt_s3_wgrad_bf16_run(const uint16_t* dyb, const uint16_t* xb, const float* dy, float* dw, float* db, void* partial, int64_t R,
                          int n, int k, int S, int accumulate, hipStream_t s);

// Attention.  q / k / v live in qkv [batch * Tp][3 C] at column offsets 0 / C / 2 C (+ 64 head), P and dP are
// [batch * heads][Tp][Tp], per-head outputs are 64-column slices of [batch * Tp][C] / [batch * Tp][3 C].
constexpr int AR_Q = 128;  // s2_attn_rows_kernel walks whole blocks of 128 query rows: rows_kernel needs Tp % AR_Q == 0
struct AttnDims {
  int batch, heads, T, Tp, C;
};
// P = softmax(scale q k^T) over the keys < T, ao = P v.  rows_kernel: s2_attn_rows_kernel<0>, else GEMM + s2_softmax
int block_attn_fwd(const AttnDims& d, const float* qkv, float* P, float* ao, float scale, bool rows_kernel, hipStream_t s);
// dqkv from dao = d ao: dV forked beside the dS chain (rowdot, then dS into dP), dq on s with dk forked beside it, joined
// before this returns.  dS: s2_attn_rows_kernel<1> (fuse_softmax_bwd && rows_kernel), the dP product's epilogue
// (fuse_softmax_bwd alone), or the plain product and s2_softmax_bwd over it
int block_attn_bwd(const AttnDims& d, const float* qkv, const float* P, const float* ao, const float* dao, float* dqkv,
                   float* dP, float* rowdot, float scale, bool rows_kernel, bool fuse_softmax_bwd, hipStream_t s);

// Residual add fused with the LayerNorm behind it, one wave per row: sum_out (may be null) = a + b, xn = LayerNorm(sum),
// per-row mean / rstd kept; rows t >= T of an image's Tp: all zero.  add_ln: a packed [batch, T, C] or padded [R, C], b null,
// pos_embed [T, C] or padded.  ls_add_ln: sum = a + ls (.) f, or a alone with ls null.  resid_ln: the block's residual
// add, LayerScale or none
int add_ln(int C, const float* a, int a_packed, const float* b, int b_is_pos, float* sum_out, const float* gamma,
           const float* beta, float* xn, float* mean, float* rstd, int T, int Tp, int R, float eps, hipStream_t s);
int ls_add_ln(int C, const float* a, const float* f, const float* ls, float* sum_out, const float* gamma, const float* beta,
              float* xn, float* mean, float* rstd, int T, int Tp, int R, float eps, hipStream_t s);
inline int resid_ln(int C, const float* a, const float* f, const float* ls, float* sum_out, const float* gamma,
                    const float* beta, float* xn, float* mean, float* rstd, int T, int Tp, int R, float eps, hipStream_t s) {
  return ls ? ls_add_ln(C, a, f, ls, sum_out, gamma, beta, xn, mean, rstd, T, Tp, R, eps, s)
            : add_ln(C, a, 0, f, 0, sum_out, gamma, beta, xn, mean, rstd, T, Tp, R, eps, s);
}

// ---- the block ----
// A block's tensors inside `params` (F = const float) or `grads` (F = float).  ls1 == ls2 == nullptr: no LayerScale (stage 2)
template <typename F>
struct BlockTensors {
  F *n1w, *n1b, *qkvw, *qkvb, *projw, *projb, *ls1, *n2w, *n2b, *fc1w, *fc1b, *fc2w, *fc2b, *ls2;
};
// base + off[i] in the order above; off holds 14 entries with_ls, else the 12 without ls1 / ls2
template <typename F>
BlockTensors<F> block_tensors(F* base, const int64_t* off, bool with_ls) {
  auto at = [&] { return base + *off++; };
  BlockTensors<F> t{};
  t.n1w = at(), t.n1b = at(), t.qkvw = at(), t.qkvb = at(), t.projw = at(), t.projb = at();
  if (with_ls) t.ls1 = at();
  t.n2w = at(), t.n2b = at(), t.fc1w = at(), t.fc1b = at(), t.fc2w = at(), t.fc2b = at();
  if (with_ls) t.ls2 = at();
  return t;
}
struct BlockActs {  // what the forward writes and the backward reads
  float *xin, *xn1, *mean1, *rstd1, *qkv, *P, *ao, *f1, *x1, *xn2, *mean2, *rstd2, *h, *a, *f2;
};
struct BlockScratch {  // one set for all blocks: the backward's gradients in flight
  float *d0, *d1, *d2, *dh, *dqkv, *dP, *acc, *wT, *rowdot;
};
struct BlockBf16 {  // stage 3's gemm_mode 1: the qkv / proj / fc1 / fc2 weights as bf16, [n, k] and transposed [k, n], and the
  uint16_t *w[4], *wt[4], *abf;  // scratch the A operand of the GEMM about to run is rounded into
  // gemm_mode 3 (aq non-null): the block's attention is the bf16 flash attention of dvt_s3_attn.hip.  The forward keeps aq =
  // bf16 (q log2(e) / 8, k, v) [3][batch * heads][Tp][64] and lse [batch * heads][Tp] of THIS block; BlockActs::qkv is then
  // fp32 scratch that only the forward touches (one buffer for all blocks), P and dP are not used
  uint16_t* aq;
  float* lse;
  // ... and qkv_db [3 C] (one for all blocks) receives the column sums of dqkv, of which the backward adds the q and v thirds
  // to the bias gradient: the k third of a qkv bias has NO gradient (a softmax row ignores a common shift of its logits), what
  // the rounded dS leaves there is noise, and AdamW would walk the k bias by a learning rate per step on it
  float* qkv_db;
  // gemm_modes 5 / 7 (xbf non-null): the weight gradients are the bf16 split-K product of dvt_s3_wgrad.hip.  xbf: the layer
  // input's row cast (abf holds dy's, which the data-gradient GEMM reads at the same time); wpart: the partial tiles, sized for
  // the largest layer (one of each for all blocks and layers: a layer's backward joins before it returns)
  uint16_t* xbf;
  void* wpart;
};
struct BlockDims {
  AttnDims ad;
  int F;  // mlp_dim
  float eps;
};
// Buffer contract: the caller has written xin and xn1 / mean1 / rstd1 = norm1(xin); block_fwd fills the rest of k and ends with
// f2 = fc2(gelu(fc1(xn2))) written and NOT added: f1 and f2 are the caller's (a block's own, or one buffer for both where no
// LayerScale gradient reads them), and the residual add of f2 with the norm behind it is the caller's resid_ln.  block_bwd
// takes d0 = d(block output), leaves d0 = d xin and uses d1, d2, dh, dqkv, dP, rowdot, wT as scratch.
// mp null: exact fp32; else forward and data-gradient GEMMs on bf16 operands, weight gradients exact all the same unless mp->xbf, and with
// mp->aq the flash attention in place of the fp32 products (rows_kernel / fuse_softmax_bwd then choose nothing).
int block_fwd(const BlockDims& d, const BlockTensors<const float>& p, const BlockActs& k, const BlockBf16* mp, bool rows_kernel,
              hipStream_t s);
int block_bwd(const BlockDims& d, const BlockTensors<const float>& p, const BlockTensors<float>& g, const BlockActs& k,
              const BlockScratch& w, const BlockBf16* mp, bool rows_kernel, bool fuse_softmax_bwd, hipStream_t s);

// Workspace carving of both steps: take() is the next piece of `base` (null: sizes only) in whole 256-byte units
struct Carver {
  char* base;
  int64_t o = 0;
  float* take(int64_t floats) {
    float* p = base ? reinterpret_cast<float*>(base + o) : nullptr;
    o += (floats * 4 + 255) / 256 * 256;
    return p;
  }
};
// R rows, C columns, F mlp columns, PP floats of P.  own_f: f1 behind ao and f2 at the end, else both left null; own_qkv
// likewise (stage 3's gemm_mode 3 points every block's qkv at one scratch buffer)
void carve_block_acts(Carver& cv, BlockActs* k, int64_t R, int64_t C, int64_t F, int64_t PP, bool own_f, bool own_qkv = true);
void carve_block_scratch(Carver& cv, BlockScratch* w, int64_t R, int64_t C, int64_t F, int64_t PP, int64_t rowdot_floats);

// ---- gemm_mode of both steps (include/dvt_stage3.h, include/dvt_stage2.h) ----
// A bit set: 1 = bf16 forward and data-gradient GEMMs, 2 = bf16 flash attention and 4 = bf16 split-K weight gradients, which
// are both built on top of bit 1
enum { MODE_GEMM = 1, MODE_ATTN = 2, MODE_WGRAD = 4 };
inline bool block_mode_ok(int mode) { return mode == 0 || mode == 1 || mode == 3 || mode == 5 || mode == 7; }
// The mode's pieces of nb blocks, which a step carves behind everything its mode 0 carves (so that mode 0 keeps its sizes):
// bit 1 every block's w / wt and one abf [R][max(3 C, F)] for all; bit 2 every block's aq [3][R][C] and lse [lse_floats =
// batch * heads * Tp] and one qkv_db [3 C]; bit 4 one xbf [R][max(F, C)] and one wpart (the largest layer's partial tiles).
// mode 0: nothing
void carve_block_bf16(Carver& cv, BlockBf16* bf, int nb, int64_t R, int64_t C, int64_t F, int64_t lse_floats, int mode);
// One block's four weight matrices of THIS call rounded into bf.w (as they lie, [n, k]) and bf.wt (transposed): `params`
// changes between steps.  The casts move 16-byte pieces: the caller checks the alignment of its arenas
int cast_block_weights(const BlockTensors<const float>& p, const BlockBf16& bf, int C, int F, hipStream_t s);
