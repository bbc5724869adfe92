// The transformer block's exact-fp32 training code that the stage-2 step (dvt_stage2.hip) and the stage-3 step
// (dvt_stage3.hip) both run, compiled once in dvt_block_train.hip.  Ordinary C++ functions, not part of the C ABI.
#pragma once
#include "dvt_common.h"

#define S2_TRY(x)               \
  do {                          \
    const int rc__ = (x);       \
    if (rc__ != 0) return rc__; \
  } while (0)

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
