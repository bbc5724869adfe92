// lab/dvt_vit_gemm8t.inc -- included by dvt_vit_gemm.hip (anonymous namespace, -DDVT_LAB only) right behind gemm_bf16_kernel_8p, whose
// macros (P8B_TILE with its MODEs 3 / 4, P8_STAGE, P8_LANE_SETUP ...) it uses.  Developer library schedule 11.
//
// RESULT (round 6, profiles/r06/r06d_*, r06e_*): bit-identical to 8p; ALONE 2.4-4.5 % faster per GEMM at 398 views (qkv 1865 ->
// 1792 us, proj 650 -> 620, fc1 2411 -> 2350, fc2 1967 -> 1920), 4.4-8 % at 110 views -- and 1.6-2.8 % SLOWER in the pipelined
// bench (2.796 against 2.849 / 2.831 images/s): a workgroup that never exits never hands its CU to the fit's row / backward
// kernels (157 KB of LDS each), which then run only between the extractor's launches.  Runs of 2-16 tiles per workgroup
// (dvt_tune_set(1, -200 - n)) with workgroup b walking b, b + grid, ... lost alone already (the resident workgroups jumped
// between distant parts of the L2-aware order, r06e); since then a generation of 256 workgroups walks CONSECUTIVE rounds of
// 256 tiles (r06g).  The product keeps one tile per workgroup.
// ---- "8t" (round 6): the same tile, the same walk, as a PERSISTENT workgroup whose tile boundary is overlapped --------------
// What a K = 768 tile pays besides its 12 k-tiles (profiles/r06/: T(K) = F + (K / 64) c over the four ViT shapes gives c = 1.41 us
// and F = 6.8-8.5 us with the bias epilogue): the dispatch gap between two workgroups of a CU (~0.9 us: the CUs are inside
// workgroups 96.7 % of a launch, profiles/r04/r04w_*), the prologue (tile map, 12 LDS-DMA issues, one cold L2 / HBM latency
// before the first MFMA and a ring that is not full for the first k-tile: 2.5-4 us) and the epilogue (3.4 us bias, 9.7 us
// GELU).  Here a workgroup walks tiles v = blockIdx.x, + gridDim.x, ...: the LAST k-tile of a tile (parity 1) stages k-tile 0
// of the NEXT tile into the parity-0 slots, one half-tile per phase; the epilogue runs in 32-row passes through the upper
// 72 KB of the LDS only (8 x 9 KB; the lower 64 KB hold the next tile's k-tile 0), and the next tile's k-loop starts on
// operands that are already there.  gfx9 retires a wave's loads AND stores in issue order on one counter: after the
// epilogue "k-tile 0 has landed" is vmcnt(20) -- the >= 16 stores of the epilogue + the two stages issued behind them are the
// only younger operations.  Round 3's "8q" did the same with a register epilogue and a static run of tiles and was no faster
// (profiles/LOG.md 5.3); differences: the LDS-staged epilogue (whole 128-B lines), the staging issued UNDER the last k-tile
// instead of behind the epilogue's store burst, the 8b walk.
template <int EPI>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_bf16_kernel_8t(GemmBArgs p) {
  constexpr int P8_AUX_A = 0, P8_AUX_B = 0;
  __shared__ __attribute__((aligned(16))) char smem[8 * EP_WAVE_BYTES];  // 136 KB: ring (128 KB) + 8 KB
  static_assert(EPI == EPI_BIAS || EPI == EPI_QKV || EPI == EPI_GELU, "epilogues with 32-row passes");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int mt = p.M / 256, nt = p.N / 256, total = mt * nt;
  // position of the current tile in the L2-aware order (map_tile): generation g = blockIdx.x / 256 walks the p.tpw x 256
  // consecutive positions from g * p.tpw * 256 in p.tpw rounds of 256 -- at any moment the resident workgroups work on ~256
  // ADJACENT tiles (shared A panels / W slices in the L2s); block b and its positions stay on XCD b % 8
  int v = ((int)blockIdx.x >> 8) * p.tpw * 256 + ((int)blockIdx.x & 255);
  int left = p.tpw;  // tiles of this workgroup still to do (incl. the current one)
  if (v >= total) return;
  const int nk = p.K / GBK;  // even, >= 4 (launch_gemm)
  TileMap tm = map_tile(v, total, mt, nt, p.group, p.mblock);
  int m0 = tm.m * 256, n0 = tm.n * 256;
  __amdgpu_buffer_rsrc_t rsA = P8_RSRC(p.A + (size_t)m0 * p.lda, 0x7fffffff);
  __amdgpu_buffer_rsrc_t rsB = P8_RSRC(p.W + (size_t)n0 * p.ldw, 0x7fffffff);
  char* const stg = smem + 65536 + wave * 9216;  // this wave's epilogue block: 32 rows x EP_LD floats = 8704 B
  {  // the first tile's k-tile 0 (every later one is staged by the tile before it)
    P8_LANE_SETUP();
    P8_STAGE(B, 0, 0, OFF_B0);
    P8_STAGE(A, 0, 0, OFF_A0);
    P8_STAGE(B, 1, 0, OFF_B1);
    P8_STAGE(A, 1, 0, OFF_A1);
  }
  bool first = true;
  f32x4 acc[8][4];
  for (;;) {
    // The k-loop's dozen per-lane constants are RE-DERIVED from the thread id at every tile (a few dozen VALU, once per
    // ~25 us): kept alive across the epilogue they are what no longer fits beside 128 accumulators + the epilogue's own
    // registers, and a spilled register is a scratch load = a vmcnt drain in the k-loop.
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    P8_LANE_SETUP();
    P8_BAR();  // (tiles after the first: every wave is done with its epilogue block -- the upper half is the ring's again)
    P8_STAGE(B, 0, 1, BUF + OFF_B0);
    P8_STAGE(A, 0, 1, BUF + OFF_A0);
    // k-tile 0 has landed: the first tile's is older than the 4 operations above; a later one is older than the previous
    // tile's epilogue (>= 16 stores) + these 4
    if (first) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
    first = false;
    P8_BAR();
    if (wm == 1) P8_BAR();  // group 1: half a phase behind through the k-loop
    // the next tile (its k-tile 0 is staged by this tile's last k-tile); none: zero-length descriptors (no memory traffic, the
    // operations still count) -- ONE straight-line body, no second code path merging behind 128 live accumulators
    const int vn = v + 256;
    --left;
    const bool more = left > 0 && vn < total;
    const TileMap tn = map_tile(more ? vn : v, total, mt, nt, p.group, p.mblock);
    const int m0n = tn.m * 256, n0n = tn.n * 256;
    const __amdgpu_buffer_rsrc_t rsAn = P8_RSRC(p.A + (size_t)m0n * p.lda, more ? 0x7fffffff : 0);
    const __amdgpu_buffer_rsrc_t rsBn = P8_RSRC(p.W + (size_t)n0n * p.ldw, more ? 0x7fffffff : 0);
    bf16x8 a[4][2], be[2][2], bo[2][2];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 2; ++j) {  // "P4 of k-tile -1": B0(0)
      be[j][0] = P8_RD(smem + OFF_B0 + j * 2048, ob0);
      be[j][1] = P8_RD(smem + OFF_B0 + j * 2048, ob1);
    }
    P8B_TILE(3, 0, 0, be, bo);
    P8B_TILE(0, 1, 1, bo, be);
    for (int t = 2; t < nk - 2; t += 2) {
      P8B_TILE(0, 0, t, be, bo);
      P8B_TILE(0, 1, t + 1, bo, be);
    }
    P8B_TILE(1, 0, nk - 2, be, bo);
    P8B_TILE(4, 1, nk - 1, bo, be);
    if (wm == 0) P8_BAR();  // balance group 1's extra barrier
    P8_BAR();               // every wave is done with the ring's upper half: it becomes epilogue space (NOT __syncthreads:
                            // its fence would wait for the LDS-DMA in flight)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4(&part)[2][4] = *reinterpret_cast<f32x4(*)[2][4]>(&acc[2 * q]);
      gemm_epilogue_lds<EPI, 2>(p, part, m0 + wm * 128 + q * 32, n0 + wn * 64, 0, 0, wave, lane, smem, stg);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the block is rewritten by the next pass
    }
    if (!more) break;
    v = vn;
    m0 = m0n;
    n0 = n0n;
    rsA = rsAn;
    rsB = rsBn;
  }
}
