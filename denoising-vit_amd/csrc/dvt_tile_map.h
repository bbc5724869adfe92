// Tile order of the bf16 GEMMs (dvt_vit_gemm.hip): blockIdx -> (m, n) tile.  Plain integer arithmetic, compiled for the device by
// dvt_vit_gemm.hip (through dvt_vit_dev.h) and for the host by the stand-alone checker of tests/test_tile_map_xcols_cpu.py (which includes this file and
// nothing else), so what the test walks IS what the kernels run.
#pragma once

#if defined(__HIPCC__)
#define DVT_TM_FN __host__ __device__ __forceinline__
#else
#define DVT_TM_FN inline
#endif

// ---- L2-aware tile rasterisation ------------------------------------------------------------
// Workgroups are dealt round-robin to the 8 XCDs (private 4 MiB L2 each), so (1) every XCD gets a
// CONTIGUOUS run of the tile order, and (2) the order walks N in groups of `group` tiles whose W
// slices (group * 128 * K * 2 B <= ~2.4 MB) stay L2-resident while all M panels stream past:
//     order = (n_group, m_panel, n_in_group)
// Plain "N fastest" re-streamed the whole W (4.7 MB for fc1/fc2 > L2) for every M panel:
// ~3.6 GB of memory-side reads per fc1 launch instead of ~0.6 GB.
struct TileMap {
  int m, n;
};
DVT_TM_FN TileMap map_tile(int bid, int nwg, int mt, int nt, int group, int mblock = 1) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
  const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;  // bijective
  const int per_group = group * mt;
  int g = id / per_group;
  const int full = nt / group;
  int width = group;
  if (g >= full) {  // last, narrower group
    g = full;
    width = nt - full * group;
  }
  const int rem = id - g * per_group;
  TileMap t;
  if (mblock <= 1) {
    t.m = rem / width;
    t.n = g * group + rem % width;
  } else {
    // (m block, n, m in block): the `mblock` tiles that share a W slab are ADJACENT in the order (they start
    // together and walk k in lock-step), and an A panel is re-touched every `mblock` ids
    const int per_block = mblock * width;
    const int mb = rem / per_block, r2 = rem - mb * per_block;
    const int left = mt - mb * mblock, hb = left < mblock ? left : mblock;
    t.n = g * group + r2 / hb;
    t.m = mb * mblock + r2 % hb;
  }
  return t;
}

// Unsigned division by a launch-invariant divisor d (1 <= d < 2^31) as multiply-high + shifts (Granlund-Montgomery, the
// round-up form): l = ceil(log2 d), m = floor(2^32 (2^l - d) / d) + 1;  x / d = (t + ((x - t) >> 1)) >> (l - 1), t = hi32(m x),
// exact for every x < 2^32 (l = 0, i.e. d = 1: m = 0, the formula degenerates -- handled).  The tile map of the 256 x 256 GEMM
// divides wave-UNIFORM values by run-time divisors four to six times per workgroup; the scalar unit has no divide, so hipcc
// expands each into ~30 VALU instructions with dependent v_rcp chains: 0.6 us from kernel entry to the first LDS-DMA issue,
// 2.4 % of a K = 768 tile (profiles/r06/r06j_*).  With these it is a handful of s_mul_hi_u32 (tests/test_kernel_math_cpu.py
// states the arithmetic; every GEMM test exercises it).
inline void fd_make(unsigned d, unsigned (&fd)[2]) {
  unsigned l = 0;
  while ((1ull << l) < d) ++l;
  fd[0] = d <= 1 ? 0u : (unsigned)((((1ull << l) - d) << 32) / d + 1);
  fd[1] = l;
}
DVT_TM_FN unsigned fd_div(unsigned x, const unsigned (&fd)[2]) {
  if (fd[1] == 0) return x;  // d = 1
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned t = __umulhi(x, fd[0]);
#else
  const unsigned t = (unsigned)(((unsigned long long)x * fd[0]) >> 32);
#endif
  return (t + ((x - t) >> 1)) >> (fd[1] - 1);
}

// The launch-invariant part of the tile order: set by tile_order_make (launch_gemm), carried in GemmBArgs
struct TileOrder {
  int group;       // N tiles per L2-resident group; with xcols > 1 the N tiles of one column set
  int mblock;      // M panels per block of the tile order (1: n fastest)
  int tiles_full;  // xcols == 1: N tiles in whole groups (nt / group * group); ids beyond take the slow path
  int xcols;       // XCD column sets: 1 (the order above), 2 or 4, a divisor of nt
  int xbase, xrem; // xcols > 1: M panels per row set (mt / nrows) and how many row sets hold one more (mt % nrows)
  // the order's divisors as multiply-shift pairs: per_group = group * mt (xcols == 1 only); per_block = mblock * group;
  // width = group; hb = mblock
  unsigned fd_pg[2], fd_pb[2], fd_w[2], fd_hb[2];
};

// The xcols a launch really runs with: the largest of {requested, requested / 2, ..., 1} that divides nt.  (With unequal
// column sets no split of M into whole row ranges balances the XCDs: the sets own different tile counts but the same number
// of XCDs each.)
inline int tile_order_xcols(int nt, int xcols) {
  int xc = xcols >= 4 ? 4 : (xcols >= 2 ? 2 : 1);
  while (xc > 1 && nt % xc) xc >>= 1;
  return xc;
}

// ---- XCD-column order (xcols = 2 or 4) -------------------------------------------------------
// Workgroup -> XCD stays blockIdx & 7.  XCD x belongs to column set x % xcols and row set x / xcols (8 / xcols row sets).  A
// column set owns nt / xcols consecutive N tiles for the WHOLE launch, so an XCD's L2 holds 1 / xcols of W (fc1 at dim 768:
// 2.4 of 4.7 MB); a row set owns a contiguous range of M panels, the first mt % nrows sets one panel more.  Inside its
// rectangle an XCD walks (m_block, n, m_in_block) as above, `group` = its N range.  Every row set walks M upwards from its
// first panel at the same pace, so the `xcols` XCDs of a row set ask for the same A panel at about the same time: one of
// them misses to HBM, the others hit the memory-side cache.
// The rectangles differ by up to one panel row (`group` tiles), while the hardware deals workgroups to the XCDs one by one:
// the grid is therefore 8 x the LARGEST rectangle (tile_order_grid), and a workgroup whose slot lies beyond its XCD's
// rectangle gets m = -1 and leaves at once.  The map is a bijection from the other workgroups onto the mt x nt tiles.
inline int tile_order_grid(const TileOrder& o, int mt, int nt) {
  if (o.xcols <= 1) return mt * nt;
  return 8 * o.group * (o.xbase + (o.xrem > 0 ? 1 : 0));
}

inline TileOrder tile_order_make(int mt, int nt, int group, int mblock, int xcols) {
  TileOrder o;
  o.xcols = tile_order_xcols(nt, xcols);
  o.group = o.xcols > 1 ? nt / o.xcols : group;
  o.mblock = mblock > 0 ? mblock : 1;
  o.tiles_full = nt / o.group * o.group;
  const int nrows = 8 / o.xcols;
  o.xbase = mt / nrows;
  o.xrem = mt % nrows;
  fd_make((unsigned)(o.group * mt), o.fd_pg);
  fd_make((unsigned)(o.mblock * o.group), o.fd_pb);
  fd_make((unsigned)o.group, o.fd_w);
  fd_make((unsigned)o.mblock, o.fd_hb);
  return o;
}

// slow path: generic divisions (ragged last M block of a rectangle)
DVT_TM_FN TileMap map_tile_xcols(const TileOrder& o, int bid) {
  const int xcd = bid & 7, loc = bid >> 3;
  const int cset = xcd & (o.xcols - 1), rset = xcd >> (o.xcols >> 1);  // xcols 2: >> 1, 4: >> 2
  const int hr = o.xbase + (rset < o.xrem ? 1 : 0);
  const int m_lo = rset * o.xbase + (rset < o.xrem ? rset : o.xrem), n_lo = cset * o.group;
  TileMap t;
  if (loc >= hr * o.group) {  // a slot beyond this XCD's rectangle: no tile
    t.m = t.n = -1;
    return t;
  }
  if (o.mblock <= 1) {
    t.m = m_lo + loc / o.group;
    t.n = n_lo + loc % o.group;
    return t;
  }
  const int per_block = o.mblock * o.group;
  const int mb = loc / per_block, r2 = loc - mb * per_block;
  const int left = hr - mb * o.mblock, hb = left < o.mblock ? left : o.mblock;
  t.n = n_lo + r2 / hb;
  t.m = m_lo + mb * o.mblock + r2 % hb;
  return t;
}

// map_tile / map_tile_xcols with the regular divisors taken from the launch arguments; ids in the last, narrower N group and
// tiles of a short last M block (rare) fall back to the generic divisions.  Same result as the slow paths for every id.
DVT_TM_FN TileMap map_tile_fast(const TileOrder& o, int bid, int nwg, int mt, int nt) {
  const int group = o.group, mblock = o.mblock;
  TileMap t;
  if (o.xcols > 1) {
    const int xcd = bid & 7, loc = bid >> 3;
    const int cset = xcd & (o.xcols - 1), rset = xcd >> (o.xcols >> 1);
    const int hr = o.xbase + (rset < o.xrem ? 1 : 0);
    if (loc >= hr * group) {
      t.m = t.n = -1;
      return t;
    }
    const int m_lo = rset * o.xbase + (rset < o.xrem ? rset : o.xrem), n_lo = cset * group;
    if (mblock <= 1) {
      const int mq = (int)fd_div((unsigned)loc, o.fd_w);
      t.m = m_lo + mq;
      t.n = n_lo + loc - mq * group;
      return t;
    }
    const int per_block = mblock * group;
    const int mb = (int)fd_div((unsigned)loc, o.fd_pb), r2 = loc - mb * per_block;
    if (hr - mb * mblock < mblock) return map_tile_xcols(o, bid);  // a short last M block
    const int nq = (int)fd_div((unsigned)r2, o.fd_hb);
    t.n = n_lo + nq;
    t.m = m_lo + mb * mblock + r2 - nq * mblock;
    return t;
  }
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
  const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;  // bijective
  const int per_group = group * mt;
  if (id >= o.tiles_full * mt) return map_tile(bid, nwg, mt, nt, group, mblock);  // the narrower last group
  const int g = (int)fd_div((unsigned)id, o.fd_pg), rem = id - g * per_group;
  if (mblock <= 1) {
    t.m = (int)fd_div((unsigned)rem, o.fd_w);
    t.n = g * group + rem - t.m * group;
    return t;
  }
  const int per_block = mblock * group;
  const int mb = (int)fd_div((unsigned)rem, o.fd_pb), r2 = rem - mb * per_block;
  if (mt - mb * mblock < mblock) return map_tile(bid, nwg, mt, nt, group, mblock);  // a short last M block
  const int nq = (int)fd_div((unsigned)r2, o.fd_hb);
  t.n = g * group + nq;
  t.m = mb * mblock + r2 - nq * mblock;
  return t;
}

// tile of position `id` in the L2-aware order of map_tile (see there): the walk of a persistent kernel
DVT_TM_FN TileMap map_tile_id(int id, int mt, int nt, int group, int mblock) {
  const int per_group = group * mt;
  int g = id / per_group;
  const int full = nt / group;
  int width = group;
  if (g >= full) {
    g = full;
    width = nt - full * group;
  }
  const int rem = id - g * per_group;
  TileMap t;
  if (mblock <= 1) {
    t.m = rem / width;
    t.n = g * group + rem % width;
  } else {
    const int per_block = mblock * width;
    const int mbk = rem / per_block, r2 = rem - mbk * per_block;
    const int left = mt - mbk * mblock, hb = left < mblock ? left : mblock;
    t.n = g * group + r2 / hb;
    t.m = mbk * mblock + r2 % hb;
  }
  return t;
}
