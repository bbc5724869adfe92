// lab/dvt_vit_lab.inc -- SUPERSEDED kernels of the bf16 extractor, kept for A/B work only.  Included by dvt_vit_gemm.hip inside
// its anonymous namespace when the library is built with -DDVT_LAB (tools/build_lab.py -> libdvt_hip_lab.so); the product
// library (libdvt_hip.so) does not contain them and dvt_tune_set rejects the values that would select them.
//   gemm_bf16_kernel_256  256x128 lock-step three-stage ring (round 1;   dvt_tune_set(1, 2))
//   gemm_bf16_kernel_sq   256x256 two-stage ring            (round 2a;  dvt_tune_set(1, 0))
// (the round-2 attention loop: lab/dvt_vit_lab_attn.inc)

// 512 threads, one workgroup per CU (144 KB LDS) = 2 waves per SIMD: allow the full 256-VGPR budget
template <int EPI>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_bf16_kernel_256(GemmBArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[3 * G2_STAGE];  // 144 KB, ONE LDS object
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const TileMap tm = map_tile(blockIdx.x, gridDim.x, p.M / G2_BM, p.N / GBN, p.group);
  const int m0 = tm.m * G2_BM, n0 = tm.n * GBN;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nk = p.K / GBK;
  // per-thread DMA source pointers (4 for the 256-row A tile, 2 for the 128-row W tile) are
  // computed once; a k-step only adds GBK elements (PMC: ~7 VALU instructions per MFMA before)
  const bf16_t* srcA[4];
  const bf16_t* srcW[2];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int s_ = it * 512 + tid, row = s_ >> 3, c = (s_ & 7) ^ (row & 7);
    srcA[it] = p.A + (size_t)(m0 + row) * p.K + c * 8;
    if (it < 2) srcW[it] = p.W + (size_t)(n0 + row) * p.K + c * 8;
  }
  const int ldsw = wave * 1024;  // this wave's 1-KB window inside each 8-KB pass
#define G2_ISSUE(kt)                                                                  \
  do {                                                                                \
    char* st_ = smem + ((kt) % 3) * G2_STAGE + ldsw;                                  \
    const int ko_ = (kt) * GBK;                                                       \
    _Pragma("unroll") for (int it = 0; it < 4; ++it)                                  \
        glds16(srcA[it] + ko_, st_ + it * 8192);                                      \
    _Pragma("unroll") for (int it = 0; it < 2; ++it)                                  \
        glds16(srcW[it] + ko_, st_ + G2_BM * GBK * 2 + it * 8192);                    \
  } while (0)
  G2_ISSUE(0);
  if (nk > 1) G2_ISSUE(1);
  for (int kt = 0; kt < nk; ++kt) {
    // retire stage kt (own loads), then meet: everyone's stage-kt data is in LDS and everyone
    // has finished reading stage kt-1, whose buffer the next issue overwrites
    if (kt + 1 < nk)
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 2 < nk) G2_ISSUE(kt + 2);
    const char* As = smem + (kt % 3) * G2_STAGE;
    const char* Bs = As + G2_BM * GBK * 2;
    // fragments of k-substep 1 are fetched while the 16 MFMAs of substep 0 issue (explicit
    // double buffer: the compiler otherwise re-uses the registers and drains lgkmcnt(0) twice
    // per substep)
    bf16x8 a0[4], b0[4], a1[4], b1[4];
    const int rowa = wm * 64 + (lane & 15), rowb = wn * 64 + (lane & 15), cg = lane >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) a0[i] = read_frag(As, rowa + i * 16, cg);
#pragma unroll
    for (int j = 0; j < 4; ++j) b0[j] = read_frag(Bs, rowb + j * 16, cg);
#pragma unroll
    for (int i = 0; i < 4; ++i) a1[i] = read_frag(As, rowa + i * 16, 4 + cg);
#pragma unroll
    for (int j = 0; j < 4; ++j) b1[j] = read_frag(Bs, rowb + j * 16, 4 + cg);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[i], b0[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[i], b1[j], acc[i][j], 0, 0, 0);
  }
#undef G2_ISSUE
  __syncthreads();  // every wave is done with the operand stages: the buffers become epilogue space
  gemm_epilogue_lds<EPI>(p, acc, m0, n0, wm, wn, wave, lane, smem);
}


// ---- 256x256x64 tile ("sq"): fewer operand bytes per flop -----------------------------------
// Ping-pong scheduling of the 256x128 kernel bought only +5 %: the k-loop is INGEST-bound.  A CU
// can keep ~100 KB of LDS-DMA in flight at ~2 us of loaded L2/MALL latency, i.e. ~16 B/clk, while
// a 256x128 tile needs 48 KB per 64-deep k-step (M*N*K*2*(1/BM + 1/BN) = 9.96 GB per fc1 launch,
// which IS its measured time).  A 256x256 tile needs 64 KB per k-step for twice the flops (-33 %
// bytes/flop).  8 waves as 2 (M) x 4 (N), each 128x64 = 8x4 MFMA accumulators (128 VGPRs); two
// 64-KB stages (prefetch distance 1, plain __syncthreads per k-tile -- the matrix pipe has slack
// once ingest is the limit); epilogue through LDS in two 64-row halves per wave.
constexpr int G4_STAGE = (256 + 256) * GBK * 2;  // 64 KB

template <int EPI>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_bf16_kernel_sq(GemmBArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[8 * EP_WAVE_BYTES];  // 136 KB >= 2 stages (128 KB)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const TileMap tm = map_tile(blockIdx.x, gridDim.x, p.M / 256, p.N / 256, p.group, p.mblock);
  const int m0 = tm.m * 256, n0 = tm.n * 256;

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nk = p.K / GBK;
  const bf16_t* srcA[4];
  const bf16_t* srcW[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int s_ = it * 512 + tid, row = s_ >> 3, c = (s_ & 7) ^ (row & 7);
    srcA[it] = p.A + (size_t)(m0 + row) * p.K + c * 8;
    srcW[it] = p.W + (size_t)(n0 + row) * p.K + c * 8;
  }
  const int ldsw = wave * 1024;
#define SQ_ISSUE(kt)                                                                  \
  do {                                                                                \
    char* st_ = smem + ((kt) & 1) * G4_STAGE + ldsw;                                  \
    const int ko_ = (kt) * GBK;                                                       \
    _Pragma("unroll") for (int it = 0; it < 4; ++it)                                  \
        glds16(srcA[it] + ko_, st_ + it * 8192);                                      \
    _Pragma("unroll") for (int it = 0; it < 4; ++it)                                  \
        glds16(srcW[it] + ko_, st_ + 32768 + it * 8192);                              \
  } while (0)
  SQ_ISSUE(0);
  __syncthreads();  // vmcnt(0) + barrier
  const int rowa = wm * 128 + (lane & 15), rowb = wn * 64 + (lane & 15), cg = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) SQ_ISSUE(kt + 1);
    const char* As = smem + (kt & 1) * G4_STAGE;
    const char* Bs = As + 32768;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 a[8], b[4];
#pragma unroll
      for (int i = 0; i < 8; ++i) a[i] = read_frag(As, rowa + i * 16, ks * 4 + cg);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = read_frag(Bs, rowb + j * 16, ks * 4 + cg);
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();  // next stage landed, everyone done reading this one
  }
#undef SQ_ISSUE
  // epilogue: two 64-row halves through this wave's LDS block
  if constexpr (EPI == EPI_RESID) {
    gemm_epilogue_resid_sq(p, acc, m0 + wm * 128, n0 + wn * 64, wave, lane, smem);
    return;
  }
  f32x4(&lo)[4][4] = *reinterpret_cast<f32x4(*)[4][4]>(&acc[0]);
  f32x4(&hi)[4][4] = *reinterpret_cast<f32x4(*)[4][4]>(&acc[4]);
  gemm_epilogue_lds<EPI>(p, lo, m0 + wm * 128, n0 + wn * 64, 0, 0, wave, lane, smem);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // own reads of the block are complete
  gemm_epilogue_lds<EPI>(p, hi, m0 + wm * 128 + 64, n0 + wn * 64, 0, 0, wave, lane, smem);
}

// ---- host side of the developer build's GEMMs: its knobs, its share of launch_gemm<EPI> and of dvt_tune_set(1, v), the debug
// buffer.  The product functions of dvt_vit_gemm.hip call these through one guarded line each.
int g_vit_tpw = 0;           // 4w kernel: target tiles per workgroup, 0 = auto (dvt_tune_set(1, -200 - n))
int g_vit_epi_abl = 0;       // dvt_tune_set(1, -560 - mask): GemmBArgs::abl
int g_vit_abl4w = 0;         // dvt_tune_set(1, -300 - mask) while a 4w schedule (6..9) is selected: its ablation mask (EPI_BIAS, timing only)
int g_vit_8p_build = 0;      // ... while schedule 5 is selected: timing build of the 8p kernel (3 stamps, 6..9 ablations; EPI_BIAS only)
unsigned* g_vit_dbg = nullptr;  // dvt_vit_debug_buffer
int g_vit_w4_grid = 0;       // dvt_tune_set(1, -600 - n): workgroups of the 4w kernel (0 = auto: a whole number per CU)

// launch_gemm<EPI>, 256 x 256 branch, in front of the product's 8p launch: true = a lab kernel of the selected schedule took
// the launch (*rc: its status); false = the product kernel is to run -- with a.abl set, as every lab launch carries it.
// grid8 = one workgroup per tile, nt = N tiles; a.ord is the xcols = 1 order here.
template <int EPI>
bool lab_launch_gemm(GemmBArgs& a, hipStream_t s, const dim3 grid8, int nt, int* rc) {
    a.abl = g_vit_epi_abl;
    const int nk = a.K / GBK;
    if constexpr (EPI == EPI_BIAS || EPI == EPI_GELU) {
      if (g_vit_gemm_variant >= 6 && g_vit_gemm_variant <= 9 && a.K >= W4_MIN_K) {
        // 4w: persistent runs of ~`tpw` tiles; the grid is a whole number of workgroups per CU
        const int tiles = (a.M / 256) * nt;
        const int tpw = g_vit_tpw > 0 ? g_vit_tpw : (nk <= 16 ? 3 : 1);
        int per_cu = (tiles + 256 * tpw - 1) / (256 * tpw);
        int nwg = 256 * (per_cu < 1 ? 1 : per_cu);
        if (g_vit_w4_grid > 0) nwg = g_vit_w4_grid;
        if (nwg > tiles) nwg = tiles;
        const dim3 grid(nwg);
        const int var = g_vit_gemm_variant - 6;  // 6: flush per tile, 7: deferred, 8: flush + fast GELU, 9: deferred + fast GELU
        bool abl_done = false;
        if constexpr (EPI == EPI_BIAS) {  // ablations (timing only, results are wrong): dvt_tune_set(1, -300 - mask)
#define W4_ABL(n) if (g_vit_abl4w == n) { hipLaunchKernelGGL((gemm_bf16_kernel_4w<EPI, 1, n>), grid, dim3(256), 0, s, a); abl_done = true; }
          W4_ABL(1) W4_ABL(2) W4_ABL(4) W4_ABL(8) W4_ABL(3) W4_ABL(5) W4_ABL(6) W4_ABL(7) W4_ABL(9) W4_ABL(14) W4_ABL(15)
#undef W4_ABL
        }
        if (abl_done) {
        } else if (var == 0) hipLaunchKernelGGL((gemm_bf16_kernel_4w<EPI, 0>), grid, dim3(256), 0, s, a);
        else if (var == 1) hipLaunchKernelGGL((gemm_bf16_kernel_4w<EPI, 1>), grid, dim3(256), 0, s, a);
        else if (var == 2) hipLaunchKernelGGL((gemm_bf16_kernel_4w<EPI, 2>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((gemm_bf16_kernel_4w<EPI, 3>), grid, dim3(256), 0, s, a);
        *rc = (int)hipGetLastError();
        return true;
      }
    }
    bool lab_done = false;
    if constexpr (EPI == EPI_BIAS) {  // the timing builds exist for the bias epilogue only (tools/lab_gemm8p_stamps.py)
      if (g_vit_gemm_variant == 5 && g_vit_8p_build != 0) {
        a.dbg = g_vit_dbg;
        switch (g_vit_8p_build) {
          case 3: hipLaunchKernelGGL((gemm_bf16_kernel_8p_lab<EPI, 3>), grid8, dim3(512), 0, s, a); break;
          case 6: hipLaunchKernelGGL((gemm_bf16_kernel_8p_lab<EPI, 6>), grid8, dim3(512), 0, s, a); break;
          case 7: hipLaunchKernelGGL((gemm_bf16_kernel_8p_lab<EPI, 7>), grid8, dim3(512), 0, s, a); break;
          case 8: hipLaunchKernelGGL((gemm_bf16_kernel_8p_lab<EPI, 8>), grid8, dim3(512), 0, s, a); break;
          default: hipLaunchKernelGGL((gemm_bf16_kernel_8p_lab<EPI, 9>), grid8, dim3(512), 0, s, a); break;
        }
        lab_done = true;
      }
    }
    if constexpr (EPI == EPI_BIAS || EPI == EPI_QKV || EPI == EPI_GELU) {
      if (!lab_done && g_vit_gemm_variant == 11 && nk >= 4 && grid8.x > 256) {  // "8t": persistent, overlapped tile boundary
        // workgroups of g_vit_tpw tiles each (0: one workgroup per CU for the whole launch); a multiple of 8 (XCD affinity)
        // generations of 256 workgroups: generation g walks tiles [g, g + 1) x tpw x 256 of the order in tpw lock-step rounds
        const int tiles = (int)grid8.x;
        a.tpw = g_vit_tpw > 0 ? g_vit_tpw : (tiles + 255) / 256;
        const int nwg = (tiles + a.tpw * 256 - 1) / (a.tpw * 256) * 256;
        hipLaunchKernelGGL((gemm_bf16_kernel_8t<EPI>), dim3(nwg), dim3(512), 0, s, a);
        lab_done = true;
      }
    }
    if (!lab_done && g_vit_gemm_variant >= 14 && g_vit_gemm_variant <= 16) {  // nt on the A (14) / W (15) / both (16) operand streams
      if (g_vit_gemm_variant == 14) hipLaunchKernelGGL((gemm_bf16_kernel_8p<EPI, false, 1>), grid8, dim3(512), 0, s, a);
      else if (g_vit_gemm_variant == 15) hipLaunchKernelGGL((gemm_bf16_kernel_8p<EPI, false, 2>), grid8, dim3(512), 0, s, a);
      else hipLaunchKernelGGL((gemm_bf16_kernel_8p<EPI, false, 3>), grid8, dim3(512), 0, s, a);
      lab_done = true;
    }
    if (!lab_done && g_vit_gemm_variant == 12) {  // the product kernel's tile anatomy (wall-clock stamps per workgroup)
      a.dbg = g_vit_dbg;
      hipLaunchKernelGGL((gemm_bf16_kernel_8p<EPI, true>), grid8, dim3(512), 0, s, a);
      lab_done = true;
    }
    if (lab_done) {
    } else if (g_vit_gemm_variant == 13) {  // round 5's walk of the ring (12 / 4 / 8 / 0 reads, run-time parity)
      hipLaunchKernelGGL((gemm_bf16_kernel_8p_lab<EPI, 0>), grid8, dim3(512), 0, s, a);
      lab_done = true;
    } else if (g_vit_gemm_variant == 10) {
      hipLaunchKernelGGL((gemm_bf16_kernel_8p_lab<EPI, 2>), grid8, dim3(512), 0, s, a);
      lab_done = true;
    } else if (g_vit_gemm_variant == 5) {
      hipLaunchKernelGGL((gemm_bf16_kernel_8p_lab<EPI, 1>), grid8, dim3(512), 0, s, a);
      lab_done = true;
    } else if (g_vit_gemm_variant == 0) {
      hipLaunchKernelGGL((gemm_bf16_kernel_sq<EPI>), grid8, dim3(512), 0, s, a);
      lab_done = true;
    }
    if (lab_done) *rc = (int)hipGetLastError();
    return lab_done;
}

// ... 256 x 128 branch, in front of the ping-pong kernel: schedule 2 = the lock-step kernel of the same tile
template <int EPI>
bool lab_launch_gemm_256(const GemmBArgs& a, hipStream_t s, int tiles, int* rc) {
  if (g_vit_gemm_variant != 2) return false;
  hipLaunchKernelGGL((gemm_bf16_kernel_256<EPI>), dim3(tiles), dim3(512), 0, s, a);
  *rc = (int)hipGetLastError();
  return true;
}

// vit_gemm_tune, where the product's chain has always asked the lab: behind its own negative keys, in front of -700 - pct,
// -100 - b and the group budget (none of which overlaps a key here).  0 / DVT_E_BADARG / VIT_TUNE_NOT_MINE.
int lab_gemm_tune(int v) {
  if ((v <= -600 && v > -700) || (v < -1100 && v >= -1100 - 65536)) {  // -600 - n (n < 100) / -1100 - n: the 4w GEMM's grid forced to n workgroups (0 = auto)
    g_vit_w4_grid = v > -700 ? -600 - v : -1100 - v;
    return 0;
  }
  if (v <= -560 && v >= -563) {  // timing-only ablation of the GEMM epilogues (GemmBArgs::abl)
    g_vit_epi_abl = -560 - v;
    return 0;
  }
  if (v <= -300 && v > -399) {  // ablation mask of the selected 4w schedule / timing build of schedule 5; anything else: neither
    const int n = -300 - v;
    g_vit_abl4w = g_vit_8p_build = 0;
    if (n == 0) return 0;
    if (g_vit_gemm_variant >= 6 && g_vit_gemm_variant <= 9) g_vit_abl4w = n;
    else if (g_vit_gemm_variant == 5 && (n == 3 || (n >= 6 && n <= 9))) g_vit_8p_build = n;
    else return DVT_E_BADARG;
    return 0;
  }
  if (v <= -200 && v > -300) {  // -200 - n: target tiles per workgroup of the 4w kernel, 0 = auto
    g_vit_tpw = -200 - v > 64 ? 64 : -200 - v;
    return 0;
  }
  if (v < 0 || v >= 16) return VIT_TUNE_NOT_MINE;  // (16 and up: the group budget in KiB, vit_gemm_tune)
  g_vit_abl4w = g_vit_8p_build = 0;  // an ablation / timing build never survives a change of schedule
  g_vit_gemm_variant = v;  // every schedule 0 .. 15 (see launch_gemm and lab_launch_gemm for the ones that name a kernel)
  return 0;
}

// dvt_vit_debug_buffer
bool lab_set_debug_buffer(void* dev_u32) {
  g_vit_dbg = static_cast<unsigned*>(dev_u32);
  return true;
}
