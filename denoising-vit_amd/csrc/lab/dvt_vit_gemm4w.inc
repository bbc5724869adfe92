// dvt_vit_gemm4w.inc -- included by dvt_vit_gemm.hip inside its anonymous namespace (GemmBArgs, map_tile_id, pack2, EPI_*).
//
// "4w": the 256 x 256 bf16 GEMM tile on FOUR waves -- one per SIMD, 128 x 128 outputs each (256 accumulator registers,
// v_mfma_f32_32x32x16_bf16) -- as a PERSISTENT workgroup whose epilogue is DEFERRED: the finished tile leaves the
// accumulators as packed bf16 (128 registers per lane) and drains to memory underneath the NEXT tile's k-loop.
//
// Why (round-3 findings, DESIGN 5 / VERDICT r3 #1).  The 8-wave kernels (8p, 8q) hold 2 x 228 registers per SIMD: nowhere
// to park a finished tile, so every tile ends with a burst of 128 KB of stores (plus the LDS round trip, plus GELU) that
// overlaps nothing on its CU: 5.6 us of a 26-us K = 768 tile for the qkv GEMM, 10.5 of 31 for fc1.  Loads and stores share
// one in-order queue per CU, so the burst also blocks the next tile's operand loads however early they are issued.  With one
// wave per SIMD the register file (512 per lane) holds accumulators (256) + parked tile (128) + fragments (56), and the
// stores go out ONE per 16 MFMAs.
//
// Data flow per workgroup (tile = 256 x 256 outputs, k-tile = 64 k, "phase" = one 64 x 64 quadrant of a wave's block over
// a k-tile = 16 MFMAs; two quadrants make a phase):
//   HBM / L2 --LDS-DMA--> ring of 8 slots x 16 KB (slot = 128 operand rows x 128 B: WHOLE lines per row -- the first version
//            of this kernel staged 64-B row pieces, twice the line requests per byte, and its DMA stream alone took 2.6 us
//            per k-tile; profiles/r04/r04c_*)
//            --ds_read_b128--> fragments --MFMA--> acc[4 m-blocks][4 n-blocks] (f32x16 each)
//   tile end:  fix-up in registers (bias, folded LayerNorm) -> parked[4][8] packed bf16
//   next tile: per phase one "unit": [GELU] -> 8 KB per-wave LDS block (transposition) -> one 1-KB store (4 output rows x
//              256 B, whole lines); 32 units = the first 8 k-tiles of the next tile
// LDS: 128 KB ring + 4 x 8 KB wave blocks = all 160 KB, ONE object (a second LDS object makes hipcc drain vmcnt).
//
// MFMA operand roles are SWAPPED (D = W_frag . A_frag: D[i][j] = sum_k W[n_i][k] A[m_j][k]), so a lane holds ONE output
// row (token m = lane & 31 of the 32-row m-block) and 16 columns per n-block; the W rows are permuted at the DMA source
// (LDS row 32 b + 8 q + 4 h + s of a wave's 128 holds W row 64 h + 16 b + 4 q + s), which makes those 64 columns
// CONTIGUOUS: lanes 0-31 own columns 0-63 of the wave's 128, lanes 32-63 columns 64-127.
//     acc[mi][nb][4 q + s] = C[mrow0 + 32 mi + (lane & 31)][ncol0 + 64 (lane >> 5) + 16 nb + 4 q + s]
//
// Ring and schedule.  A k-tile is four slots: A_lo / A_hi = the rows of m-blocks {0, 1} / {2, 3} of BOTH wave rows,
// W_lo / W_hi = n-blocks {0, 1} / {2, 3} of both wave columns; two parities.  A PHASE is two quadrants = 32 MFMAs:
//   phase    quadrants           W fragments (streamed, 2 per k-step)   A fragments (held: 8)            LDS-DMA issued
//   PA(t)    (lo,lo), (lo,hi)    W_lo(t), then W_hi(t)                  A_lo(t); reads A_hi(t)           W_lo(t+1), W_hi(t+1)
//   PB(t)    (hi,hi), (hi,lo)    W_hi(t), then W_lo(t)                  A_hi(t); reads A_lo(t+1)         A_lo(t+2), A_hi(t+2)
// A fragments roll: once k-step ks of a phase's second quadrant has been multiplied, its two registers are re-loaded with
// the NEXT half's k-step ks (the last one through a spare pair, so that every read of a phase is issued before the barrier
// that ends it).  W fragments are read twice per k-tile (1.5 x the minimal LDS traffic, what 8p moves too) -- holding them
// would cost 64 more registers.  Every slot is re-staged in the phase after its last reader; the shortest issue-to-use
// distance is two phases = one k-tile.  (The first cut had one quadrant per phase: four barriers per k-tile cost 0.2 us of
// 1.6, profiles/r04/r04e_*.)
//
// Synchronisation: ONE s_barrier per phase, at the start of its last k-step: s_waitcnt lgkmcnt(0) [this wave's reads of
// the phase are complete], s_waitcnt vmcnt(10) [its DMAs older than this phase's have landed], s_barrier [everyone's].
// vmcnt is counted, never 0 inside the loop: gfx9 retires loads and stores of a wave in issue order, and EVERY phase
// issues the same ten vector-memory operations -- two "aux" operations (one per quadrant) and eight DMAs (a quarter of
// two slots).  An aux operation is a deferred unit's store (quadrants 0-31 of a tile), a parameter DMA (quadrants 32-34:
// LayerNorm statistics, bias, column sums -> the wave's LDS block) or a store through a zero-length descriptor (dropped by
// the range check: no memory traffic, but it keeps the count).  The k-tile counter runs THROUGH tile boundaries: the last
// two k-tiles of a tile stage the first two of the next one (its buffer descriptor; a zero-length one when there is none).

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned w4_u32x4 __attribute__((ext_vector_type(4)));
typedef int w4_i32x4 __attribute__((ext_vector_type(4)));

constexpr int W4_SLOT = 16384;               // 128 operand rows x 64 k bf16
constexpr int W4_RING = 8 * W4_SLOT;         // 2 parities x {A_lo, W_lo, W_hi, A_hi} = 128 KB
constexpr int W4_STG = 8192;                 // per-wave transposition block: 32 rows x 256 B
constexpr int W4_LDS = W4_RING + 4 * W4_STG; // 160 KB
constexpr int W4_MIN_K = 640;                // nk >= 10: the parameter DMAs of phases 32-34 are older than the last 15 operations at the tile end
enum { W4_A_LO = 0, W4_W_LO = 1, W4_W_HI = 2, W4_A_HI = 3 };  // slot kinds of one parity

// A cheaper GELU for the deferred epilogue (VAR bit 1, opt-in; the default is the .hip file's gelu_erf, exact to 1.5e-7):
// x * sigmoid(2 u), u = x (c1 + c3 x^2), fitted to 0.5 x (1 + erf(x / sqrt 2)) on [-8, 8] (tools/fit_gelu.py: max abs
// deviation 2.7e-4 at |x| ~ 2.9 against 4.7e-4 for the textbook tanh form).  6 VALU, two of them transcendental, instead of 14.
constexpr float W4_GELU_C1 = 2.308765411e+00f, W4_GELU_C3 = 1.001256108e-01f;  // 2 log2(e) folded in: the kernel uses exp2
__device__ __forceinline__ float w4_gelu_fast(float x) {
  const float w = fmaf(x * x, W4_GELU_C3, W4_GELU_C1);
  const float e = __builtin_amdgcn_exp2f(-x * w);  // exp(-2 u)
  return x * __builtin_amdgcn_rcpf(1.0f + e);
}

#define W4_RSRC(ptr, len) __builtin_amdgcn_make_buffer_rsrc((void*)(ptr), 0, (len), 0x00020000)

// ABL: timing-only ablations (1 no DMA, 2 no MFMA, 4 no fragment reads, 8 no barrier / wait); VAR bit 0: deferred epilogue
// (the product; 0 = every tile is flushed at its end, bring-up / A-B); bit 1: w4_gelu_fast
template <int EPI, int VAR, int ABL = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void gemm_bf16_kernel_4w(GemmBArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[W4_LDS];  // ONE LDS object
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1, h = lane >> 5, l31 = lane & 31;
  const int mt = p.M / 256, nt = p.N / 256, ntiles = mt * nt;
  // Workgroup -> tiles.  XCD x owns a contiguous range of the tile order (private L2); its workgroups arrive in
  // "generations" of 32 (one per CU), and the 32 workgroups of a generation walk their block of the range in ROUNDS of 32
  // consecutive tiles: tile = start_x + 32 (round) + (local id % 32).  At any moment the CUs of an XCD therefore work on ~32
  // ADJACENT tiles, which share A panels and W slices through the L2 -- runs of consecutive tiles per workgroup (the first
  // version) spread an XCD over ~10 M panels at once and halved the DMA stream's rate (profiles/r04/r04d_*).
  int tile0, tstride, count;
  {
    const int nwg = gridDim.x, bid = blockIdx.x, xcd = bid & 7, loc = bid >> 3;
    const int nx = nwg < 8 ? nwg : 8;                            // XCDs that get workgroups (block b runs on XCD b % 8)
    const int tq = ntiles / nx, tr = ntiles % nx;
    const int start_x = xcd * tq + (xcd < tr ? xcd : tr), tiles_x = tq + (xcd < tr ? 1 : 0);
    const int wg_x = (nwg >> 3) + (xcd < (nwg & 7) ? 1 : 0);     // workgroups of this XCD
    const int g = loc >> 5, r = loc & 31;                        // generation, lane in it
    const int w_g = min(32, wg_x - 32 * g);                      // its width (the last one may be narrower)
    // the generation's block of the XCD's range: proportional to the workgroups before / in it
    const int b0 = (int)((long long)tiles_x * (32 * g) / wg_x), b1 = (int)((long long)tiles_x * (32 * g + w_g) / wg_x);
    tile0 = start_x + b0 + r;
    tstride = w_g;
    count = (b1 - b0 - r + w_g - 1) / w_g;  // tiles b0 + r, b0 + r + w_g, ... below b1
  }
  if (count <= 0) return;
#define W4_TILE(I) (tile0 + tstride * (I))
  const int nk = p.K >> 6;  // k-tiles per tile
  const bool has_ln = (IS_QKV(EPI) || IS_GELU(EPI)) && p.ln_stats != nullptr;
  const int lda2 = p.lda * 2, ldw2 = p.ldw * 2;

  // ---- per-lane constants ----------------------------------------------------------------------------------------
  // DMA: instruction j = 4 wave + jj of a slot fills LDS rows 8 j + (lane >> 3), 16-B position (lane & 7); a row stores its
  // logical chunk c at position c ^ ((row >> 1) & 7) (bank swizzle, applied at the source): (row >> 1) & 7 = 4 (jj & 1) |
  // (lane >> 4), i.e. two per-lane source offsets per operand, 64 B apart in the XOR sense.  The rest of the source row is
  // scalar.  LDS row rho = 64 g + lam of a slot (g: wave row / column, lam = 8 (j & 7) + (lane >> 3)):
  //   A half a: tile row 128 g + 64 a + lam
  //   W half a: lam = 32 bl + 8 q + 4 hh + s holds W row 128 g + 64 hh + 16 (2 a + bl) + 4 q + s; here bl = (j & 7) >> 2,
  //             q = j & 3, hh = lane >> 5, s = (lane >> 3) & 3
  //   (re-derived from the lane id where they are used, like the epilogue's addresses below: W4_VOA / W4_VOW)
#define W4_VOA(L) (((L) >> 3) * lda2 + ((((L) & 7) ^ ((L) >> 4)) << 4))
#define W4_VOW(L) ((64 * ((L) >> 5) + (((L) >> 3) & 3)) * ldw2 + ((((L) & 7) ^ ((L) >> 4)) << 4))
  // fragment reads: row 64 g + 32 bl + l31 of a slot, logical chunk 2 ks + h at position (2 ks + h) ^ ((l31 >> 1) & 7):
  // one XOR with ks << 5 on the k-step-0 address
  const int sw = (l31 >> 1) & 7;
  const int fa0 = (64 * wm + l31) * 128 + ((h ^ sw) << 4), fw0 = (64 * wn + l31) * 128 + ((h ^ sw) << 4);
  char* const stg = smem + W4_RING + wave * W4_STG;  // this wave's transposition block (and parameter block, phases 32-34)
  // transposition block: a lane writes its row l31, logical 16-B chunk 8 h + cc at position (8 h + cc) ^ (l31 & 15):
  // byte offset stw ^ (cc << 4) -- the block is 256-B aligned, so the chunk's low three bits are an XOR on one register --
  // and reads row 4 uu + g4, chunk l15 at position l15 ^ (row & 15) = (l15 ^ g4) ^ 4 (uu & 3): str ^ ((uu & 3) << 6), + 1 KB
  // per uu as the instruction's immediate offset.  These (and the units' store offsets) are RE-DERIVED from the lane id at
  // every use (a handful of VALU per phase): kept in registers they are the dozen that no longer fits beside 256 accumulators
  // + 128 parked + 56 fragment registers, and a spilled register is a scratch load = s_waitcnt vmcnt(0) in this loop.
  const int g4 = lane >> 4, l15 = lane & 15;
  const int stg_off = W4_RING + wave * W4_STG;
#define W4_LANE_OPAQUE(x) int x = lane; asm volatile("" : "+v"(x))
#define W4_STW(L) (stg_off + ((L) & 31) * 256 + ((((8 * ((L) >> 5)) ^ ((L) & 8)) | ((L) & 7)) << 4))
#define W4_STR(L) (stg_off + ((L) >> 4) * 256 + ((((L) & 15) ^ ((L) >> 4)) << 4))

  struct Src {
    __amdgpu_buffer_rsrc_t a, b;
  };
  auto src_of = [&](int id, bool valid, int& m0, int& n0) {
    const TileMap tm = map_tile_id(valid ? id : tile0, mt, nt, p.group, p.mblock);
    m0 = tm.m * 256;
    n0 = tm.n * 256;
    const int len = valid ? 0x7fffffff : 0;  // no tile: every access is out of range (no memory traffic)
    Src s;
    s.a = W4_RSRC(p.A + (size_t)m0 * p.lda, len);
    s.b = W4_RSRC(p.W + (size_t)n0 * p.ldw, len);
    return s;
  };

#define W4_DMA(RS, VO, SOFF, DST)                                                                    \
  do {                                                                                               \
    if constexpr (!(ABL & 1)) __builtin_amdgcn_raw_ptr_buffer_load_lds(RS, (lds_ptr_t)(DST), 16, VO, SOFF, 0, 0); \
  } while (0)
  // instruction JJ (0..3) of this wave's quarter of a slot: operand ISW (0 A, 1 W), half HALF, tile-local k-tile KT (KT >= nk:
  // the next tile's k-tile KT - nk), to LDS byte offset DSTB
#define W4_STAGE1(ISW, HALF, KT, DSTB, JJ, CHK)                                                      \
  do {                                                                                               \
    const bool nx_ = (CHK) && (KT) >= nk;  /* CHK = 0: the caller knows KT < nk (nk >= 10) */         \
    const int kb_ = ((nx_ ? (KT) - nk : (KT)) << 7);                                                 \
    const int j_ = wave * 4 + (JJ);                                                                  \
    const int so_ = (ISW) ? (128 * (j_ >> 3) + 32 * (HALF) + 16 * ((j_ & 7) >> 2) + 4 * (j_ & 3)) * ldw2 \
                          : (128 * (j_ >> 3) + 64 * (HALF) + 8 * (j_ & 7)) * lda2;                   \
    const __amdgpu_buffer_rsrc_t rs_ = (ISW) ? (nx_ ? nxt.b : cur.b) : (nx_ ? nxt.a : cur.a);        \
    W4_DMA(rs_, ((ISW) ? W4_VOW(ld_) : W4_VOA(ld_)) ^ (((JJ) & 1) << 6), so_ + kb_,                  \
           smem + (DSTB) + j_ * 1024);                                                               \
  } while (0)
  // the aux operation of a phase that has nothing to store: dropped by the range check, counted by vmcnt
#define W4_DUMMY_AUX() __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(w4_i32x4, unit_v), rs_null, 0, 0, 0)
#define W4_SB(PAR, KIND) (((((PAR) & 1) << 2) + (KIND)) * W4_SLOT)

  const __amdgpu_buffer_rsrc_t rs_null = W4_RSRC(p.out, 0);
  w4_u32x4 unit_v;  // the unit in flight between its LDS read (previous phase) and its store
  asm volatile("" : "=v"(unit_v));
  int m0, n0, m1 = 0, n1 = 0;
  Src cur = src_of(W4_TILE(0), true, m0, n0);
  Src nxt = src_of(W4_TILE(1), 1 < count, m1, n1);
  // prologue: k-tile 0 whole, then what PB of "k-tile -1" issues in the steady state (two aux, A_lo and A_hi of k-tile 1)
  const int ld_ = lane;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) W4_STAGE1(0, 0, 0, W4_SB(0, W4_A_LO), jj, 0);
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) W4_STAGE1(1, 0, 0, W4_SB(0, W4_W_LO), jj, 0);
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) W4_STAGE1(1, 1, 0, W4_SB(0, W4_W_HI), jj, 0);
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) W4_STAGE1(0, 1, 0, W4_SB(0, W4_A_HI), jj, 0);
  W4_DUMMY_AUX();
  W4_DUMMY_AUX();
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) W4_STAGE1(0, 0, 1, W4_SB(1, W4_A_LO), jj, 0);
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) W4_STAGE1(0, 1, 1, W4_SB(1, W4_A_HI), jj, 0);

  f32x16 acc[4][4];
  bf16x8 af[2][4], asp[2], wf[2][2];  // A fragments of the current half [m-block][k-step], the rolling spare, W stream [buffer][n-block]
  w4_u32x4 parked[4][8];              // the previous tile: packed bf16, [m-block][16-B chunk = 8 columns]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) asm volatile("" : "=v"(parked[i][j]));  // "defined", no instruction: nothing is parked yet

  // fragment (BL, KS) of the A / W half in the slot at byte offset SB
#define W4_RD(F, SB, BL, KS)                                                                         \
  ((ABL & 4) ? (bf16x8){(short)((F) ^ ((KS) << 5)), 1, 2, 3, 4, 5, 6, (short)(BL)}                   \
             : *reinterpret_cast<const bf16x8*>(smem + (SB) + ((F) ^ ((KS) << 5)) + (BL) * 4096))
#define W4_MFMA4(MIH, NBH, KS, WBUF, FIRST_)                                                         \
  do {                                                                                               \
    if constexpr (ABL & 2) {                                                                         \
      _Pragma("unroll") for (int b_ = 0; b_ < 2; ++b_) {                                             \
        asm volatile("" ::"v"(af[b_][KS]));                                                          \
        asm volatile("" ::"v"(wf[WBUF][b_]));                                                        \
      }                                                                                              \
      if (FIRST_) {                                                                                  \
        _Pragma("unroll") for (int mi_ = 0; mi_ < 2; ++mi_)                                          \
        _Pragma("unroll") for (int nb_ = 0; nb_ < 2; ++nb_)                                          \
        _Pragma("unroll") for (int e_ = 0; e_ < 16; ++e_) acc[2 * (MIH) + mi_][2 * (NBH) + nb_][e_] = 0.f; \
      }                                                                                              \
      break;                                                                                         \
    }                                                                                                \
    _Pragma("unroll") for (int mi_ = 0; mi_ < 2; ++mi_)                                              \
    _Pragma("unroll") for (int nb_ = 0; nb_ < 2; ++nb_)                                              \
        acc[2 * (MIH) + mi_][2 * (NBH) + nb_] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(             \
            wf[WBUF][nb_], af[mi_][KS],                                                              \
            (FIRST_) ? (f32x16){0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f} \
                     : acc[2 * (MIH) + mi_][2 * (NBH) + nb_], 0, 0, 0);                              \
  } while (0)
  // One quadrant (16 MFMAs).  MIH / NBH: which; WB: byte offset of its W slot, NWB: of the NEXT quadrant's; ROLL: re-load the
  // A fragments behind the multiplications from the slot at RB; S0 .. S3: the LDS-DMA issued in k-steps 0 .. 3; AUX: the
  // quadrant's aux operation; BAR: the phase ends here (barrier at the start of the last k-step; S3 must be empty).
#define W4_QUAD(MIH, NBH, WB, NWB, ROLL, RB, FIRST_, AUX, S0, S1, S2, S3, BAR)                       \
  do {                                                                                               \
    int fa_ = fa0, fw_ = fw0, ld_ = lane;                                                            \
    asm volatile("" : "+v"(fa_), "+v"(fw_), "+v"(ld_));  /* opaque: per-quadrant address arithmetic, not hoisted registers */ \
    /* k-step 0 */                                                                                   \
    wf[1][0] = W4_RD(fw_, WB, 0, 1);                                                                 \
    wf[1][1] = W4_RD(fw_, WB, 1, 1);                                                                 \
    AUX;                                                                                             \
    S0;                                                                                              \
    W4_MFMA4(MIH, NBH, 0, 0, FIRST_);                                                                \
    if (ROLL) {                                                                                      \
      af[0][0] = W4_RD(fa_, RB, 0, 0);                                                               \
      af[1][0] = W4_RD(fa_, RB, 1, 0);                                                               \
    }                                                                                                \
    /* k-step 1 */                                                                                   \
    wf[0][0] = W4_RD(fw_, WB, 0, 2);                                                                 \
    wf[0][1] = W4_RD(fw_, WB, 1, 2);                                                                 \
    S1;                                                                                              \
    W4_MFMA4(MIH, NBH, 1, 1, false);                                                                 \
    if (ROLL) {                                                                                      \
      af[0][1] = W4_RD(fa_, RB, 0, 1);                                                               \
      af[1][1] = W4_RD(fa_, RB, 1, 1);                                                               \
    }                                                                                                \
    /* k-step 2 */                                                                                   \
    wf[1][0] = W4_RD(fw_, WB, 0, 3);                                                                 \
    wf[1][1] = W4_RD(fw_, WB, 1, 3);                                                                 \
    S2;                                                                                              \
    if (ROLL) {                                                                                      \
      asp[0] = W4_RD(fa_, RB, 0, 3);                                                                 \
      asp[1] = W4_RD(fa_, RB, 1, 3);                                                                 \
    }                                                                                                \
    W4_MFMA4(MIH, NBH, 2, 0, false);                                                                 \
    if (ROLL) {                                                                                      \
      af[0][2] = W4_RD(fa_, RB, 0, 2);                                                               \
      af[1][2] = W4_RD(fa_, RB, 1, 2);                                                               \
    }                                                                                                \
    /* k-step 3 (BAR: every read of this phase is out; barrier); the next quadrant's first W fragments */ \
    if constexpr ((BAR) && !(ABL & 8)) {                                                             \
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                             \
      asm volatile("s_waitcnt vmcnt(10)" ::: "memory");                                              \
      __builtin_amdgcn_sched_barrier(0);                                                             \
      __builtin_amdgcn_s_barrier();                                                                  \
    }                                                                                                \
    if (BAR) __builtin_amdgcn_sched_barrier(0);                                                      \
    S3;                                                                                              \
    wf[0][0] = W4_RD(fw_, NWB, 0, 0);                                                                \
    wf[0][1] = W4_RD(fw_, NWB, 1, 0);                                                                \
    W4_MFMA4(MIH, NBH, 3, 1, false);                                                                 \
    if (ROLL) {                                                                                      \
      af[0][3] = asp[0];                                                                             \
      af[1][3] = asp[1];                                                                             \
    }                                                                                                \
  } while (0)
#define W4_NONE ((void)0)
#define W4_ST2(SW, SH, ST, DB, J0, J1, CHK) do { W4_STAGE1(SW, SH, ST, DB, J0, CHK); W4_STAGE1(SW, SH, ST, DB, J1, CHK); } while (0)
  // One k-tile = two phases of two quadrants; G = global k-tile counter (slot parity), kt = tile-local index.
  //   PA(t): (lo, lo), (lo, hi)  stages W_lo(t+1), W_hi(t+1) -> the other parity;  reads A_hi(t) behind the second quadrant
  //   PB(t): (hi, hi), (hi, lo)  stages A_lo(t+2), A_hi(t+2) -> this parity;       reads A_lo(t+1) behind the second quadrant
#define W4_KTILE(FIRST_, AUX1, AUX2, AUX3, AUX4, CHK)                                                \
  do {                                                                                               \
    const int pb_ = (G & 1) * 4 * W4_SLOT, qb_ = pb_ ^ (4 * W4_SLOT);                                \
    W4_QUAD(0, 0, pb_ + W4_W_LO * W4_SLOT, pb_ + W4_W_HI * W4_SLOT, false, 0, FIRST_, AUX1,          \
            W4_ST2(1, 0, kt + 1, qb_ + W4_W_LO * W4_SLOT, 0, 1, CHK),                                \
            W4_STAGE1(1, 0, kt + 1, qb_ + W4_W_LO * W4_SLOT, 2, CHK),                                \
            W4_STAGE1(1, 0, kt + 1, qb_ + W4_W_LO * W4_SLOT, 3, CHK),                                \
            W4_STAGE1(1, 1, kt + 1, qb_ + W4_W_HI * W4_SLOT, 0, CHK), 0);                            \
    W4_QUAD(0, 1, pb_ + W4_W_HI * W4_SLOT, pb_ + W4_W_HI * W4_SLOT, true, pb_ + W4_A_HI * W4_SLOT, FIRST_, AUX2, \
            W4_STAGE1(1, 1, kt + 1, qb_ + W4_W_HI * W4_SLOT, 1, CHK),                                \
            W4_STAGE1(1, 1, kt + 1, qb_ + W4_W_HI * W4_SLOT, 2, CHK),                                \
            W4_STAGE1(1, 1, kt + 1, qb_ + W4_W_HI * W4_SLOT, 3, CHK), W4_NONE, 1);                   \
    W4_QUAD(1, 1, pb_ + W4_W_HI * W4_SLOT, pb_ + W4_W_LO * W4_SLOT, false, 0, FIRST_, AUX3,          \
            W4_ST2(0, 0, kt + 2, pb_ + W4_A_LO * W4_SLOT, 0, 1, CHK),                                \
            W4_STAGE1(0, 0, kt + 2, pb_ + W4_A_LO * W4_SLOT, 2, CHK),                                \
            W4_STAGE1(0, 0, kt + 2, pb_ + W4_A_LO * W4_SLOT, 3, CHK),                                \
            W4_STAGE1(0, 1, kt + 2, pb_ + W4_A_HI * W4_SLOT, 0, CHK), 0);                            \
    W4_QUAD(1, 0, pb_ + W4_W_LO * W4_SLOT, qb_ + W4_W_LO * W4_SLOT, true, qb_ + W4_A_LO * W4_SLOT, FIRST_, AUX4, \
            W4_STAGE1(0, 1, kt + 2, pb_ + W4_A_HI * W4_SLOT, 1, CHK),                                \
            W4_STAGE1(0, 1, kt + 2, pb_ + W4_A_HI * W4_SLOT, 2, CHK),                                \
            W4_STAGE1(0, 1, kt + 2, pb_ + W4_A_HI * W4_SLOT, 3, CHK), W4_NONE, 1);                   \
    ++G;                                                                                             \
    ++kt;                                                                                            \
  } while (0)

  // ---- output side ------------------------------------------------------------------------------------------------
  // unit (mi, uu) of the parked tile: rows 32 mi + 4 uu + g4 of the wave's block, bytes 16 l15 of the 256-B row piece
  __amdgpu_buffer_rsrc_t o_rs = rs_null;  // the parked tile's 128 x 128 block (zero length while nothing is parked)
  int o_ld2 = 0;                          // its row pitch in bytes
  // m-block MI of `parked` -> the wave's LDS block (8 x 16 B per lane)
#define W4_PARK_WRITE(MI)                                                                            \
  do {                                                                                               \
    W4_LANE_OPAQUE(l_);                                                                              \
    const int w_ = W4_STW(l_);  /* the eight addresses are one XOR each */                           \
    _Pragma("unroll") for (int cc_ = 0; cc_ < 8; ++cc_)                                              \
        *reinterpret_cast<w4_u32x4*>(smem + (w_ ^ (cc_ << 4))) = parked[MI][cc_];                    \
  } while (0)
  // unit UU (rows 4 UU + g4 of the block in LDS) -> unit_v
#define W4_UNIT_READ(UU)                                                                             \
  do {                                                                                               \
    W4_LANE_OPAQUE(l_);                                                                              \
    const int r_ = W4_STR(l_);                                                                       \
    unit_v = *reinterpret_cast<const w4_u32x4*>(smem + (r_ ^ (((UU) & 3) << 6)) + (UU) * 1024);      \
  } while (0)
  // unit_v = unit (MI, UU): [GELU], one 16-B store
#define W4_UNIT_STORE(MI, UU, RS)                                                                    \
  do {                                                                                               \
    w4_u32x4 v_ = unit_v;                                                                            \
    if constexpr (IS_GELU(EPI)) {                                                                    \
      _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) {                                             \
        const float xl_ = __uint_as_float(v_[e_] << 16);          /* (no top-level commas: this macro is a macro argument) */ \
        const float xh_ = __uint_as_float(v_[e_] & 0xffff0000u);                                     \
        const float lo_ = (VAR & 2) ? w4_gelu_fast(xl_) : gelu_erf(xl_);                             \
        const float hi_ = (VAR & 2) ? w4_gelu_fast(xh_) : gelu_erf(xh_);                             \
        v_[e_] = pack2(lo_, hi_);                                                                    \
      }                                                                                              \
    }                                                                                                \
    int so_ = (32 * (MI) + 4 * (UU)) * o_ld2;                                                        \
    asm volatile("" : "+s"(so_));  /* opaque: the 32 unit offsets are not hoisted into 32 registers */ \
    W4_LANE_OPAQUE(l_);                                                                              \
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(w4_i32x4, v_), RS,                     \
                                           (l_ >> 4) * o_ld2 + (l_ & 15) * 16 + so_, 0, 0);          \
  } while (0)
  // the aux operation of window phase U (0..31): store unit U (read one phase earlier), then read unit U + 1 (after
  // writing its m-block to the LDS block when it is the first of one)
#define W4_WIN_AUX(U)                                                                                \
  do {                                                                                               \
    W4_UNIT_STORE((U) >> 3, (U) & 7, o_rs);                                                          \
    if ((U) < 31) {                                                                                  \
      if ((((U) + 1) & 7) == 0) W4_PARK_WRITE(((U) + 1) >> 3);                                       \
      W4_UNIT_READ(((U) + 1) & 7);                                                                   \
    }                                                                                                \
  } while (0)

  // ---- the stream -------------------------------------------------------------------------------------------------
  int G = 0;  // global k-tile counter (slot parity = G & 1)
  asm volatile("s_waitcnt vmcnt(10)" ::: "memory");  // k-tile 0 has landed (everything but the last phase's ten operations)
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  kernarg_ptr_t kp = (kernarg_ptr_t)__builtin_amdgcn_kernarg_segment_ptr();
  for (int ti = 0; ti < count; ++ti) {
    int kt = 0;
    // the fragments P1 starts from are read HERE, not by the previous tile's last phase: 40 fewer live registers across the
    // fix-up (where the accumulators meet the parked tile), for one exposed LDS latency per tile
    {
      const int pb_ = (G & 1) * 4 * W4_SLOT;
      int fa_ = fa0, fw_ = fw0;
      asm volatile("" : "+v"(fa_), "+v"(fw_));
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        af[0][ks] = W4_RD(fa_, pb_ + W4_A_LO * W4_SLOT, 0, ks);
        af[1][ks] = W4_RD(fa_, pb_ + W4_A_LO * W4_SLOT, 1, ks);
      }
      wf[0][0] = W4_RD(fw_, pb_ + W4_W_LO * W4_SLOT, 0, 0);
      wf[0][1] = W4_RD(fw_, pb_ + W4_W_LO * W4_SLOT, 1, 0);
    }
    // the window: phases 0-31 carry the 32 units of the parked tile (through a zero-length descriptor when there is none),
    // fully unrolled -- the m-block index is a register index
    W4_KTILE(true, W4_WIN_AUX(0), W4_WIN_AUX(1), W4_WIN_AUX(2), W4_WIN_AUX(3), 0);
    W4_KTILE(false, W4_WIN_AUX(4), W4_WIN_AUX(5), W4_WIN_AUX(6), W4_WIN_AUX(7), 0);
    W4_KTILE(false, W4_WIN_AUX(8), W4_WIN_AUX(9), W4_WIN_AUX(10), W4_WIN_AUX(11), 0);
    W4_KTILE(false, W4_WIN_AUX(12), W4_WIN_AUX(13), W4_WIN_AUX(14), W4_WIN_AUX(15), 0);
    W4_KTILE(false, W4_WIN_AUX(16), W4_WIN_AUX(17), W4_WIN_AUX(18), W4_WIN_AUX(19), 0);
    W4_KTILE(false, W4_WIN_AUX(20), W4_WIN_AUX(21), W4_WIN_AUX(22), W4_WIN_AUX(23), 0);
    W4_KTILE(false, W4_WIN_AUX(24), W4_WIN_AUX(25), W4_WIN_AUX(26), W4_WIN_AUX(27), 0);
    W4_KTILE(false, W4_WIN_AUX(28), W4_WIN_AUX(29), W4_WIN_AUX(30), W4_WIN_AUX(31), 0);
    // phases 32-34: the epilogue's parameters travel to the wave's LDS block (free again: the window is over) as aux
    // operations -- the rows' LayerNorm statistics (128 x (mean, rstd) -> bytes [0, 1 KB)), bias (256 columns from the
    // wave's first one -> [1 KB, 2 KB)) and the folded LayerNorm's column sums ([2 KB, 3 KB)).  An absent parameter is a
    // zero-length descriptor: zeros land, no branch anywhere.  (Columns past N are out of range as well: zeros.)
    {
      const int ncol0 = n0 + wn * 128;
      const __amdgpu_buffer_rsrc_t rs_st = W4_RSRC(has_ln ? (const void*)(p.ln_stats + m0 + wm * 128) : (const void*)p.out,
                                                   has_ln ? 1024 : 0);
      const __amdgpu_buffer_rsrc_t rs_bi = W4_RSRC(p.bias != nullptr ? (const void*)(p.bias + ncol0) : (const void*)p.out,
                                                   p.bias != nullptr ? (p.N - ncol0) * 4 : 0);
      const __amdgpu_buffer_rsrc_t rs_cs = W4_RSRC(has_ln ? (const void*)(p.ln_cs + ncol0) : (const void*)p.out,
                                                   has_ln ? (p.N - ncol0) * 4 : 0);
      W4_KTILE(false, W4_DMA(rs_st, lane * 16, 0, stg), W4_DMA(rs_bi, lane * 16, 0, stg + 1024),
               W4_DMA(rs_cs, lane * 16, 0, stg + 2048), W4_DUMMY_AUX(), 1);
    }
    // the rest of the tile; its last two k-tiles stage the next tile
    while (kt < nk) W4_KTILE(false, W4_DUMMY_AUX(), W4_DUMMY_AUX(), W4_DUMMY_AUX(), W4_DUMMY_AUX(), 1);

    // ---- tile boundary: this tile becomes `parked`, the next one `cur` ----------------------------------------------
    {
      // fix-up in registers: acc (+ bias | folded LayerNorm) -> parked, from the parameters in the wave's LDS block:
      //   rstd * (acc - mean * cs) + b'  =  rstd * acc - (rstd * mean) * cs + b'      (no LayerNorm: rstd = 1, cs = 0)
      // The four columns of a register quad are a 16-B LDS read (the same address for the 32 lanes of a half: broadcast).
      // (hipcc pads nothing inside asm: the last MFMAs' results must have left the matrix pipe before the asm reads below)
      asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
      W4_LANE_OPAQUE(lf_);  // (the two per-lane addresses below are derived here, not kept across the k-loop)
      float mu[4], rs[4];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const float2 st = *reinterpret_cast<const float2*>(smem + stg_off + (32 * mi + (lf_ & 31)) * 8);
        rs[mi] = has_ln ? st.y : 1.0f;
        mu[mi] = has_ln ? -st.x * st.y : 0.0f;  // -(rstd * mean)
      }
      const char* const colp = smem + stg_off + 1024 + (lf_ >> 5) * 256;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        float4 bq[4], cq[4];  // bias / column sums of the lane's 16 columns of n-block nb
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          bq[q] = *reinterpret_cast<const float4*>(colp + (16 * nb + 4 * q) * 4);
          cq[q] = *reinterpret_cast<const float4*>(colp + 1024 + (16 * nb + 4 * q) * 4);
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
          // ONE accumulator tuple at a time (asm: with plain reads hipcc copies ~200 accumulators out at the loop exit and
          // spills): left alone the scheduler hoists all 256 reads to the top of the fix-up
          float t[16];
#pragma unroll
          for (int e = 0; e < 16; ++e) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(t[e]) : "a"(acc[mi][nb][e]));
          w4_u32x4 lo, hi;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float v0 = fmaf(rs[mi], t[4 * q + 0], fmaf(mu[mi], cq[q].x, bq[q].x));
            const float v1 = fmaf(rs[mi], t[4 * q + 1], fmaf(mu[mi], cq[q].y, bq[q].y));
            const float v2 = fmaf(rs[mi], t[4 * q + 2], fmaf(mu[mi], cq[q].z, bq[q].z));
            const float v3 = fmaf(rs[mi], t[4 * q + 3], fmaf(mu[mi], cq[q].w, bq[q].w));
            if (q < 2) {
              lo[2 * q] = pack2(v0, v1);
              lo[2 * q + 1] = pack2(v2, v3);
            } else {
              hi[2 * q - 4] = pack2(v0, v1);
              hi[2 * q - 3] = pack2(v2, v3);
            }
          }
          parked[mi][2 * nb] = lo;      // columns 16 nb .. + 7 of the lane's half
          parked[mi][2 * nb + 1] = hi;  // columns 16 nb + 8 .. + 15
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      asm volatile("" : "+s"(kp));  // opaque: the loads below are not hoisted above the k-loop
      const int ldo = IS_QKV(EPI) ? 2 * kp->dim : kp->N;
      o_ld2 = ldo * 2;
      const __amdgpu_buffer_rsrc_t rs_out = W4_RSRC(kp->out + (size_t)(m0 + wm * 128) * ldo + n0 + wn * 128, 0x7fffffff);
      if constexpr (!(VAR & 1)) {  // bring-up / A-B: every unit at once, at every tile end
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
          W4_PARK_WRITE(mi);
#pragma unroll
          for (int uu = 0; uu < 8; ++uu) {
            W4_UNIT_READ(uu);
            W4_UNIT_STORE(mi, uu, rs_out);
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the block is rewritten by the next m-block
        }
        // (32 stores sit behind the next tile's DMAs: drain, so that the counted waits stay exact)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      } else {
        o_rs = rs_out;
        W4_PARK_WRITE(0);  // (the parameters in the block have been consumed)
        W4_UNIT_READ(0);
      }
    }
    cur = nxt;
    m0 = m1;
    n0 = n1;
    nxt = src_of(W4_TILE(ti + 2), ti + 2 < count, m1, n1);
  }
  if constexpr (VAR & 1) {  // the run's last tile is still parked (its first m-block already in the LDS block, unit 0 read)
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      if (mi > 0) W4_PARK_WRITE(mi);
#pragma unroll
      for (int uu = 0; uu < 8; ++uu) {
        if (mi > 0 || uu > 0) W4_UNIT_READ(uu);
        W4_UNIT_STORE(mi, uu, o_rs);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the block is rewritten by the next m-block
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stores above and the (empty) DMAs of the non-existent next tile
#undef W4_KTILE
#undef W4_QUAD
#undef W4_NONE
#undef W4_ST2
#undef W4_MFMA4
#undef W4_RD
#undef W4_STAGE1
#undef W4_DMA
#undef W4_DUMMY_AUX
#undef W4_SB
#undef W4_PARK_WRITE
#undef W4_UNIT_READ
#undef W4_UNIT_STORE
#undef W4_WIN_AUX
#undef W4_TILE
#undef W4_VOA
#undef W4_VOW
#undef W4_LANE_OPAQUE
#undef W4_STW
#undef W4_STR
}
