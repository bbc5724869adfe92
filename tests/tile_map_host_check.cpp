// Stand-alone host program of tests/test_tile_map_xcols_cpu.py: walks the tile order of csrc/dvt_tile_map.h -- the very
// functions the 256 x 256 GEMM kernel runs -- for the cases named on the command line and writes every id's tile to stdout.
//   usage: tile_map_host_check mt nt xcols mblock group [mt nt xcols mblock group ...]
//   output (int32, native endian) per case: grid, effective xcols, then grid x {fast m, fast n, slow m, slow n}
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dvt_tile_map.h"

int main(int argc, char** argv) {
  if (argc < 6 || (argc - 1) % 5) {
    std::fprintf(stderr, "usage: %s mt nt xcols mblock group [...]\n", argv[0]);
    return 2;
  }
  for (int a = 1; a + 4 < argc; a += 5) {
    const int mt = std::atoi(argv[a]), nt = std::atoi(argv[a + 1]), xcols = std::atoi(argv[a + 2]);
    const int mblock = std::atoi(argv[a + 3]), group = std::atoi(argv[a + 4]);
    const TileOrder o = tile_order_make(mt, nt, group, mblock, xcols);
    const int grid = tile_order_grid(o, mt, nt);
    std::vector<int> out;
    out.reserve(2 + 4 * (size_t)grid);
    out.push_back(grid);
    out.push_back(o.xcols);
    for (int bid = 0; bid < grid; ++bid) {
      const TileMap f = map_tile_fast(o, bid, grid, mt, nt);
      const TileMap s = o.xcols > 1 ? map_tile_xcols(o, bid) : map_tile(bid, grid, mt, nt, o.group, o.mblock);
      out.push_back(f.m);
      out.push_back(f.n);
      out.push_back(s.m);
      out.push_back(s.n);
    }
    if (std::fwrite(out.data(), sizeof(int), out.size(), stdout) != out.size()) return 1;
  }
  return 0;
}
