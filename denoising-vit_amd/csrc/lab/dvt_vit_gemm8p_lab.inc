// lab/dvt_vit_gemm8p_lab.inc -- the re-schedules and timing builds of the product's 8-phase GEMM (dvt_vit_gemm.hip,
// gemm_bf16_kernel_8p): SM 1 "8m", 2 "8h", 3 cycle stamps, 6..9 ablations with WRONG results.  Included by dvt_vit_gemm.hip
// inside #ifdef DVT_LAB only; the product library has none of it.  SM = 0 here is the product schedule again (the body the
// variants were derived from) and is never launched.  tools/lab_gemm8p_stamps.py, tools/lab_gemm8p.py drive it.
template <int MODE, int SM>  // 0 steady state, 1 tile nk-2 (no issue in P3/P4), 2 tile nk-1 (no issue)
struct P8WaitLab;
template <> struct P8WaitLab<0, 0> { static constexpr int w1 = 8, w2 = 8, w4 = 8; };
template <> struct P8WaitLab<1, 0> { static constexpr int w1 = 8, w2 = 8, w4 = 4; };
template <> struct P8WaitLab<2, 0> { static constexpr int w1 = 2, w2 = 0, w4 = -1; };
// SM = 1 ("8m", lab build, dvt_tune_set(1, 5)): the half-tile of a phase is staged in the MIDDLE OF ITS MFMA SEGMENT instead of in the load
// segment, i.e. AFTER the phase's counted wait instead of before it -- the same issue order, every wait one stage (2
// instructions) tighter.  WAR: the slot is re-staged even later than before.  RAW: unchanged (the waits still precede the
// second barrier of the phase before the one that reads).  SM = 2 "8h": see P8H_TILE.  SM = 3, 6..9: timing builds.
template <> struct P8WaitLab<0, 1> { static constexpr int w1 = 6, w2 = 6, w4 = 6; };
template <> struct P8WaitLab<1, 1> { static constexpr int w1 = 6, w2 = 6, w4 = 4; };
template <> struct P8WaitLab<2, 1> { static constexpr int w1 = 2, w2 = 0, w4 = -1; };
template <> struct P8WaitLab<0, 3> : P8WaitLab<0, 0> {};
template <> struct P8WaitLab<1, 3> : P8WaitLab<1, 0> {};
template <> struct P8WaitLab<2, 3> : P8WaitLab<2, 0> {};
template <> struct P8WaitLab<0, 6> : P8WaitLab<0, 0> {};
template <> struct P8WaitLab<1, 6> : P8WaitLab<1, 0> {};
template <> struct P8WaitLab<2, 6> : P8WaitLab<2, 0> {};
template <> struct P8WaitLab<0, 7> : P8WaitLab<0, 0> {};
template <> struct P8WaitLab<1, 7> : P8WaitLab<1, 0> {};
template <> struct P8WaitLab<2, 7> : P8WaitLab<2, 0> {};
template <> struct P8WaitLab<0, 8> : P8WaitLab<0, 0> {};
template <> struct P8WaitLab<1, 8> : P8WaitLab<1, 0> {};
template <> struct P8WaitLab<2, 8> : P8WaitLab<2, 0> {};
template <> struct P8WaitLab<0, 9> : P8WaitLab<0, 0> {};
template <> struct P8WaitLab<1, 9> : P8WaitLab<1, 0> {};
template <> struct P8WaitLab<2, 9> : P8WaitLab<2, 0> {};

// the same 16 MFMAs with MID (a DMA stage, or nothing) between the two k-steps
#define P8_MFMA2(IB, JB, AF, BF, MID)                                                             \
  do {                                                                                            \
    __builtin_amdgcn_s_setprio(1);                                                                \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                 \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                 \
        acc[IB + i][JB + j] =                                                                     \
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(AF[i][0], BF[j][0], acc[IB + i][JB + j], 0, 0, 0); \
    __builtin_amdgcn_sched_barrier(0);                                                            \
    MID;                                                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                            \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                 \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                 \
        acc[IB + i][JB + j] =                                                                     \
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(AF[i][1], BF[j][1], acc[IB + i][JB + j], 0, 0, 0); \
    __builtin_amdgcn_s_setprio(0);                                                                \
  } while (0)

template <int EPI, int SM>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_bf16_kernel_8p_lab(GemmBArgs p) {
  unsigned long long entry_t_ = 0;
  if constexpr (SM >= 3) entry_t_ = __builtin_readcyclecounter();
  __shared__ __attribute__((aligned(16))) char smem[8 * EP_WAVE_BYTES];  // 136 KB >= 8 half-tiles (128 KB)
  // De-synchronised start (dvt_tune_set(1, -700 - pct)).  A launch begins with one workgroup per CU, all tiles cost the same,
  // so the CUs walk through k-loop and epilogue in LOCK STEP for the whole launch: every ~26 us all 256 of them burst their
  // 128 KB of output at the memory system together (the chip's store rate, 5-6 TB/s: the bias epilogue's 5.6 us) and then
  // nobody stores for 20 us.  The workgroups of the first round therefore wait a hash-spread fraction of one tile time
  // (s_memrealtime, 100 MHz); every later workgroup inherits its CU's phase.  Results do not depend on it.
  if (p.stagger_ticks > 0 && blockIdx.x < 256) {
    const unsigned h_ = ((unsigned)blockIdx.x * 2654435761u) >> 16;  // 16-bit hash of the block id
    const unsigned long long wait_ = ((unsigned long long)p.stagger_ticks * h_) >> 16;
    const unsigned long long t0_ = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0_ < wait_) __builtin_amdgcn_s_sleep(16);
  }
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
  // DMA sources: [half][pass]; one pass = 512 threads x 16 B = 64 rows of a half-tile
  const bf16_t* srcA[2][2];
  const bf16_t* srcB[2][2];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int s_ = it * 512 + tid, r = s_ >> 3, c = (s_ & 7) ^ (r & 7);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      srcA[h][it] = p.A + (size_t)(m0 + (r >> 6) * 128 + h * 64 + (r & 63)) * p.lda + c * 8;
      srcB[h][it] = p.W + (size_t)(n0 + (r >> 5) * 64 + h * 32 + (r & 31)) * p.ldw + c * 8;
    }
  }
  constexpr int OFF_A0 = 0, OFF_A1 = 16384, OFF_B0 = 32768, OFF_B1 = 49152, BUF = 65536;
  char* const ldsw = smem + wave * 1024;
#define P8_STAGE(SRC, kt, off)                                   \
  do {                                                           \
    glds16(SRC[0] + (size_t)(kt) * GBK, ldsw + (off));           \
    glds16(SRC[1] + (size_t)(kt) * GBK, ldsw + (off) + 8192);    \
  } while (0)
  // fragment read offsets inside a half-tile: row*128 + ((ks*4 + cg) ^ (row & 7))*16
  const int cg = lane >> 4;
  const int ra = wm * 64 + (lane & 15), rb = wn * 32 + (lane & 15);
  const int oa0 = ra * 128 + (((0 + cg) ^ (ra & 7)) << 4), oa1 = ra * 128 + (((4 + cg) ^ (ra & 7)) << 4);
  const int ob0 = rb * 128 + (((0 + cg) ^ (rb & 7)) << 4), ob1 = rb * 128 + (((4 + cg) ^ (rb & 7)) << 4);
#define P8_RD(base, off) (*reinterpret_cast<const bf16x8*>((base) + (off)))

  // prologue: A0 B0 B1 A1 of tile 0, A0 B0 of tile 1 -- the order the steady state continues
  P8_STAGE(srcA[0], 0, OFF_A0);
  P8_STAGE(srcB[0], 0, OFF_B0);
  P8_STAGE(srcB[1], 0, OFF_B1);
  P8_STAGE(srcA[1], 0, OFF_A1);
  P8_STAGE(srcA[0], 1, BUF + OFF_A0);
  P8_STAGE(srcB[0], 1, BUF + OFF_B0);
  if constexpr (SM == 2) wait_vm<6>();  // (its first load segment reads B1 of tile 0 as well)
  else wait_vm<8>();
  P8_BAR();
  if (wm == 1) P8_BAR();  // group 1: half a phase behind from here on

  bf16x8 a[4][2], b0[2][2], b1[2][2];
  // SM >= 6: ablation builds for tools/lab_gemm8p_stamps.py (timing only, results wrong): 6 = no LDS-DMA inside the k-loop, 7 = 6 +
  // the ring parity frozen (compile-time fragment-read addresses), 8 = the kernel as it is (k-loop cycles only), 9 = no fragment reads
  constexpr bool NO_DMA = SM == 6 || SM == 7, NO_PARITY = SM == 7, NO_READS = SM == 9;
  if constexpr (NO_READS) {
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i][0] = a[i][1] = (bf16x8){1, 2, 3, 4, 5, 6, 7, 8};
#pragma unroll
    for (int j = 0; j < 2; ++j) b0[j][0] = b0[j][1] = b1[j][0] = b1[j][1] = (bf16x8){1, 2, 3, 4, 5, 6, 7, 8};
  }
  // SM == 3, the timing build: s_memtime after each of the 8 barriers of k-tiles 4 and 5 (shader cycles; wave-uniform SGPRs)
  unsigned st[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) st[i] = 0u;
#define P8_STAMP(t, i)                                                              \
  do {                                                                              \
    if constexpr (SM == 3) {                                                        \
      unsigned long long t64_;                                                      \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t64_)::"memory");   \
      __builtin_amdgcn_sched_barrier(0);                                            \
      const unsigned now_ = (unsigned)t64_;                                         \
      st[i] = (t) == 4 ? now_ : st[i];                                              \
      if ((i) == 0) st[13] = (t) == 5 ? now_ : st[13];                              \
    }                                                                               \
  } while (0)
#define P8_TILE(MODE, t)                                                                          \
  do {                                                                                            \
    const int bo_ = NO_PARITY ? 0 : ((t) & 1) * BUF, bn_ = bo_ ^ BUF;                             \
    const char* base_ = smem + bo_;                                                               \
    /* P1 */                                                                                      \
    if (!NO_READS) _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                \
      b0[j][0] = P8_RD(base_ + OFF_B0 + j * 2048, ob0);                                           \
      b0[j][1] = P8_RD(base_ + OFF_B0 + j * 2048, ob1);                                           \
    }                                                                                             \
    if (!NO_READS) _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                \
      a[i][0] = P8_RD(base_ + OFF_A0 + i * 2048, oa0);                                            \
      a[i][1] = P8_RD(base_ + OFF_A0 + i * 2048, oa1);                                            \
    }                                                                                             \
    if (MODE == 0) P8_STAMP(t, 8);  /* (its lgkmcnt(0): the 12 fragment reads have COMPLETED) */   \
    if (MODE <= 1 && SM != 1 && !NO_DMA) P8_STAGE(srcB[1], (t) + 1, bn_ + OFF_B1);                               \
    if (MODE == 0) P8_STAMP(t, 9);                                                                \
    if (!NO_DMA) wait_vm<P8WaitLab<MODE, SM>::w1>();                                                                  \
    if (MODE == 0) P8_STAMP(t, 10);                                                               \
    P8_BAR();                                                                                     \
    if (MODE == 0) P8_STAMP(t, 0);                                                            \
    P8_LGKM0();                                                                                   \
    if constexpr (SM == 1 && MODE <= 1) P8_MFMA2(0, 0, a, b0, P8_STAGE(srcB[1], (t) + 1, bn_ + OFF_B1)); \
    else P8_MFMA(0, 0, a, b0);                                                                    \
    if (MODE == 0) P8_STAMP(t, 11);  /* 16 MFMAs issued */                                         \
    P8_BAR();                                                                                     \
    if (MODE == 0) P8_STAMP(t, 1);                                                            \
    /* P2 */                                                                                      \
    if (!NO_READS) _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                \
      b1[j][0] = P8_RD(base_ + OFF_B1 + j * 2048, ob0);                                           \
      b1[j][1] = P8_RD(base_ + OFF_B1 + j * 2048, ob1);                                           \
    }                                                                                             \
    if (MODE <= 1 && SM != 1 && !NO_DMA) P8_STAGE(srcA[1], (t) + 1, bn_ + OFF_A1);                               \
    if (!NO_DMA) wait_vm<P8WaitLab<MODE, SM>::w2>();                                                                  \
    P8_BAR();                                                                                     \
    if (MODE == 0) P8_STAMP(t, 2);                                                            \
    P8_LGKM0();                                                                                   \
    if constexpr (SM == 1 && MODE <= 1) P8_MFMA2(0, 2, a, b1, P8_STAGE(srcA[1], (t) + 1, bn_ + OFF_A1)); \
    else P8_MFMA(0, 2, a, b1);                                                                    \
    P8_BAR();                                                                                     \
    if (MODE == 0) P8_STAMP(t, 3);                                                            \
    /* P3 */                                                                                      \
    if (!NO_READS) _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                \
      a[i][0] = P8_RD(base_ + OFF_A1 + i * 2048, oa0);                                            \
      a[i][1] = P8_RD(base_ + OFF_A1 + i * 2048, oa1);                                            \
    }                                                                                             \
    if (MODE == 0 && SM != 1 && !NO_DMA) P8_STAGE(srcA[0], (t) + 2, bo_ + OFF_A0);                               \
    P8_BAR();                                                                                     \
    if (MODE == 0) P8_STAMP(t, 4);                                                            \
    P8_LGKM0();                                                                                   \
    if constexpr (SM == 1 && MODE == 0) P8_MFMA2(4, 2, a, b1, P8_STAGE(srcA[0], (t) + 2, bo_ + OFF_A0)); \
    else P8_MFMA(4, 2, a, b1);                                                                    \
    P8_BAR();                                                                                     \
    if (MODE == 0) P8_STAMP(t, 5);                                                            \
    /* P4 */                                                                                      \
    if (MODE == 0 && SM != 1 && !NO_DMA) P8_STAGE(srcB[0], (t) + 2, bo_ + OFF_B0);                               \
    if (!NO_DMA) wait_vm<P8WaitLab<MODE, SM>::w4>();                                                                  \
    P8_BAR();                                                                                     \
    if (MODE == 0) P8_STAMP(t, 6);                                                            \
    if constexpr (SM == 1 && MODE == 0) P8_MFMA2(4, 0, a, b0, P8_STAGE(srcB[0], (t) + 2, bo_ + OFF_B0)); \
    else P8_MFMA(4, 0, a, b0);                                                                    \
    P8_BAR();                                                                                     \
    if (MODE == 0) P8_STAMP(t, 7);                                                            \
  } while (0)

// SM == 2 ("8h", dvt_tune_set(1, 10)): the same ring and the same issue order on TWO phases per k-tile instead of
// four -- X = {reads B0 B1 A0; stage B1(t+1) A1(t+1); wait [A1(t)]} 32 MFMAs (A0,B0) (A0,B1);  Y = {reads A1; stage A0(t+2)
// B0(t+2); wait [B1(t+1) and older]} 32 MFMAs (A1,B1) (A1,B0) -- i.e. four barriers per k-tile and MFMA segments of 512 cycles.
// Hazards as in the four-phase walk: a slot is re-staged a full phase (two barriers) or more after the load segments that read
// it; a half-tile is read in the load segment after the one whose counted wait covered it.
#define P8H_TILE(MODE, t)                                                                         \
  do {                                                                                            \
    const int bo_ = ((t) & 1) * BUF, bn_ = bo_ ^ BUF;                                             \
    const char* base_ = smem + bo_;                                                               \
    /* X */                                                                                       \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                               \
      b0[j][0] = P8_RD(base_ + OFF_B0 + j * 2048, ob0);                                           \
      b0[j][1] = P8_RD(base_ + OFF_B0 + j * 2048, ob1);                                           \
    }                                                                                             \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                               \
      a[i][0] = P8_RD(base_ + OFF_A0 + i * 2048, oa0);                                            \
      a[i][1] = P8_RD(base_ + OFF_A0 + i * 2048, oa1);                                            \
    }                                                                                             \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                               \
      b1[j][0] = P8_RD(base_ + OFF_B1 + j * 2048, ob0);                                           \
      b1[j][1] = P8_RD(base_ + OFF_B1 + j * 2048, ob1);                                           \
    }                                                                                             \
    if (MODE <= 1) {                                                                              \
      P8_STAGE(srcB[1], (t) + 1, bn_ + OFF_B1);                                                   \
      P8_STAGE(srcA[1], (t) + 1, bn_ + OFF_A1);                                                   \
      wait_vm<8>();                                                                               \
    } else {                                                                                      \
      wait_vm<0>();                                                                               \
    }                                                                                             \
    P8_BAR();                                                                                     \
    P8_LGKM0();                                                                                   \
    P8_MFMA(0, 0, a, b0);                                                                         \
    P8_MFMA(0, 2, a, b1);                                                                         \
    P8_BAR();                                                                                     \
    /* Y */                                                                                       \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                               \
      a[i][0] = P8_RD(base_ + OFF_A1 + i * 2048, oa0);                                            \
      a[i][1] = P8_RD(base_ + OFF_A1 + i * 2048, oa1);                                            \
    }                                                                                             \
    if (MODE == 0) {                                                                              \
      P8_STAGE(srcA[0], (t) + 2, bo_ + OFF_A0);                                                   \
      P8_STAGE(srcB[0], (t) + 2, bo_ + OFF_B0);                                                   \
      wait_vm<6>();                                                                               \
    } else if (MODE == 1) {                                                                       \
      wait_vm<2>();                                                                               \
    }                                                                                             \
    P8_BAR();                                                                                     \
    P8_LGKM0();                                                                                   \
    P8_MFMA(4, 2, a, b1);                                                                         \
    P8_MFMA(4, 0, a, b0);                                                                         \
    P8_BAR();                                                                                     \
  } while (0)

  unsigned long long loop_t0_ = 0;
  if constexpr (SM >= 3) loop_t0_ = __builtin_readcyclecounter();
  int t = 0;
  if constexpr (SM == 2) {
    for (; t < nk - 2; ++t) P8H_TILE(0, t);
    P8H_TILE(1, t);
    ++t;
    P8H_TILE(2, t);
  } else {
    for (; t < nk - 2; ++t) P8_TILE(0, t);
    P8_TILE(1, t);
    ++t;
    P8_TILE(2, t);
  }
#undef P8H_TILE
#undef P8_TILE
#undef P8_STAGE
#undef P8_RD
#undef P8_STAMP
  if constexpr (SM >= 3) {
    const unsigned loop_cyc_ = (unsigned)(__builtin_readcyclecounter() - loop_t0_);
    if (p.dbg != nullptr && lane == 0 && (wave & 3) == 0) {
      unsigned* d_ = p.dbg + ((size_t)blockIdx.x * 2 + wm) * 24;  // 24 u32 per (workgroup, wave group): 0..13 stamps, 16..21 below
#pragma unroll
      for (int i = 0; i < 14; ++i) d_[i] = st[i];
      d_[20] = loop_cyc_;  // the whole k-loop of this tile (nk k-tiles)
      d_[21] = (unsigned)nk;
    }
  }
  if (wm == 0) P8_BAR();  // balance group 1's extra barrier
  __syncthreads();        // operand buffers become epilogue space
  if constexpr (EPI == EPI_RESID) {
    gemm_epilogue_resid_sq(p, acc, m0 + wm * 128, n0 + wn * 64, wave, lane, smem);
    return;
  }
  f32x4(&lo)[4][4] = *reinterpret_cast<f32x4(*)[4][4]>(&acc[0]);
  f32x4(&hi)[4][4] = *reinterpret_cast<f32x4(*)[4][4]>(&acc[4]);
  gemm_epilogue_lds<EPI>(p, lo, m0 + wm * 128, n0 + wn * 64, 0, 0, wave, lane, smem);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  gemm_epilogue_lds<EPI>(p, hi, m0 + wm * 128 + 64, n0 + wn * 64, 0, 0, wave, lane, smem);
  if constexpr (SM >= 3) {  // ticks from kernel entry to the last store issued AND retired
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned total_ = (unsigned)(__builtin_readcyclecounter() - entry_t_);
    if (p.dbg != nullptr && lane == 0 && (wave & 3) == 0) {
      unsigned* d_ = p.dbg + ((size_t)blockIdx.x * 2 + wm) * 24;
      d_[19] = total_;
      d_[18] = (unsigned)entry_t_;                                    // absolute tick of the kernel entry (low 32 bits)
      d_[17] = __builtin_amdgcn_s_getreg((31 << 11) | 4);             // HW_REG_HW_ID: wave / simd / cu / sh / se
      d_[16] = __builtin_amdgcn_s_getreg((31 << 11) | 20);            // HW_REG_XCC_ID
    }
  }
}
