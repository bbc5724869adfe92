"""The tile order of the 256 x 256 bf16 GEMM (csrc/dvt_tile_map.h: map_tile, map_tile_xcols, map_tile_fast) without a GPU.

The header is plain integer arithmetic, so a stand-alone host program (tests/tile_map_host_check.cpp, its own main, built
here with the host compiler of hipcc) walks the SAME functions the kernel runs; this file restates the order in Python -- the
grouped order of rounds 2-6 transcribed as it stood before the XCD column sets, the column order from its definition (each
XCD's rectangle enumerated, not computed id by id) -- and compares.

XCD x = blockIdx & 7 belongs to column set x % xcols and row set x // xcols.  A requested xcols that does not divide the N
tile count is halved until it does (tile_order_xcols): with unequal column sets the XCD loads cannot balance, the sets own
different tile counts and the same number of XCDs.  The grid is 8 x the largest rectangle; slots beyond an XCD's rectangle
map to (-1, -1) and the workgroup leaves.
"""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "denoising-vit_amd" / "csrc"

MTS = [1, 2, 7, 8, 9, 43, 2129]
NTS = [1, 3, 6, 9, 12, 16, 24]
XCOLS = [1, 2, 4]
MBLOCKS = [1, 4]


def groups_of(nt):
    """N tiles per group for the xcols = 1 order: one group (the default at K = 768) and a width that leaves a narrower last
    group where nt allows (the slow path of map_tile_fast)."""
    return sorted({nt, min(nt, 5)})


def parent_map(bid, nwg, mt, nt, group, mblock):
    """map_tile as it stood before the column sets (rounds 2-6), id for id."""
    q, r, xcd, loc = nwg >> 3, nwg & 7, bid & 7, bid >> 3
    i = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + loc
    per_group = group * mt
    g = i // per_group
    full = nt // group
    width = group
    if g >= full:
        g, width = full, nt - full * group
    rem = i - g * per_group
    if mblock <= 1:
        return rem // width, g * group + rem % width
    per_block = mblock * width
    mb, r2 = divmod(rem, per_block)
    hb = min(mblock, mt - mb * mblock)
    return mb * mblock + r2 % hb, g * group + r2 // hb


def effective_xcols(nt, xcols):
    while xcols > 1 and nt % xcols:
        xcols //= 2
    return xcols


def rectangle(x, mt, nt, xc):
    """(m_lo, m_hi, n_lo, n_hi) of XCD x: contiguous ranges, remainders of M spread over the first row sets."""
    nrows = 8 // xc
    cset, rset = x % xc, x // xc
    base, rem = divmod(mt, nrows)
    m_lo = rset * base + min(rset, rem)
    w = nt // xc
    return m_lo, m_lo + base + (1 if rset < rem else 0), cset * w, (cset + 1) * w


def xcols_walk(x, mt, nt, xc, mblock):
    """The tiles of XCD x in the order it walks them: (m block, n, m in block) inside its rectangle."""
    m_lo, m_hi, n_lo, n_hi = rectangle(x, mt, nt, xc)
    out = []
    for mb in range(m_lo, m_hi, mblock):
        for n in range(n_lo, n_hi):
            for m in range(mb, min(mb + mblock, m_hi)):
                out.append((m, n))
    return out


@pytest.fixture(scope="module")
def host_maps(tmp_path_factory):
    """{(mt, nt, xcols, mblock, group): (grid, effective xcols, int32 [grid, 4] = fast m, n, slow m, n)} from the host program."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = tmp_path_factory.mktemp("tile_map") / "tile_map_host_check"
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}",
                    str(ROOT / "tests" / "tile_map_host_check.cpp"), "-o", str(exe)], check=True)
    cases = [(mt, nt, xc, mb, g) for mt in MTS for nt in NTS for xc in XCOLS for mb in MBLOCKS
             for g in (groups_of(nt) if xc == 1 else [nt])]
    res = {}
    for i in range(0, len(cases), 64):  # (argv stays short)
        chunk = cases[i:i + 64]
        raw = subprocess.run([str(exe)] + [str(v) for c in chunk for v in c], check=True, capture_output=True).stdout
        buf = np.frombuffer(raw, dtype=np.int32)
        pos = 0
        for c in chunk:
            grid, xc_eff = int(buf[pos]), int(buf[pos + 1])
            res[c] = (grid, xc_eff, buf[pos + 2:pos + 2 + 4 * grid].reshape(grid, 4))
            pos += 2 + 4 * grid
        assert pos == buf.size
    return res


def test_all_cases_ran(host_maps):
    assert len(host_maps) == sum(len(MTS) * len(MBLOCKS) * (len(groups_of(nt)) + 2) for nt in NTS)


def test_fast_path_equals_slow_path(host_maps):
    for c, (_, _, t) in host_maps.items():
        assert np.array_equal(t[:, :2], t[:, 2:]), f"fast != slow for (mt, nt, xcols, mblock, group) = {c}"


def test_map_is_a_bijection_onto_the_tiles(host_maps):
    for (mt, nt, xc, mb, g), (grid, _, t) in host_maps.items():
        live = t[t[:, 0] >= 0]
        assert bool((t[t[:, 0] < 0] == -1).all())
        ids = np.sort(live[:, 0].astype(np.int64) * nt + live[:, 1])
        assert np.array_equal(ids, np.arange(mt * nt)), f"not a bijection: {(mt, nt, xc, mb, g)}"
        assert bool((live[:, 1] >= 0).all()) and bool((live[:, 1] < nt).all())


def test_xcols_1_is_the_parent_order(host_maps):
    for (mt, nt, xc, mb, g), (grid, xc_eff, t) in host_maps.items():
        if xc != 1:
            continue
        assert grid == mt * nt and xc_eff == 1
        if mt > 43:  # the Python loop: every id of the small grids, a stride of the large one plus its two ends
            ids = sorted(set(range(0, grid, 37)) | set(range(64)) | set(range(grid - 64, grid)))
        else:
            ids = range(grid)
        for bid in ids:
            assert tuple(t[bid, :2]) == parent_map(bid, grid, mt, nt, g, mb), f"{(mt, nt, mb, g)} id {bid}"


def test_effective_xcols_and_grid(host_maps):
    for (mt, nt, xc, mb, g), (grid, xc_eff, _) in host_maps.items():
        assert xc_eff == effective_xcols(nt, xc)
        if xc_eff > 1:
            nrows = 8 // xc_eff
            assert grid == 8 * (nt // xc_eff) * -(-mt // nrows)
            assert grid % 8 == 0 and mt * nt <= grid < mt * nt + 8 * (nt // xc_eff)


def test_each_xcd_walks_its_rectangle_in_block_order(host_maps):
    """Every tile of XCD x lies in its rectangle, and the walk is (m block, n, m in block) with all row sets going up."""
    for (mt, nt, xc, mb, g), (grid, xc_eff, t) in host_maps.items():
        if xc_eff == 1:
            continue
        for x in range(8):
            mine = t[x::8, :2]
            want = xcols_walk(x, mt, nt, xc_eff, mb)
            assert len(want) <= len(mine)
            assert bool((mine[len(want):] == -1).all()), "slots beyond the rectangle are not idle"
            if want:
                assert np.array_equal(mine[:len(want)], np.array(want, dtype=np.int32)), f"{(mt, nt, xc, mb)} XCD {x}"
                m_lo, m_hi, n_lo, n_hi = rectangle(x, mt, nt, xc_eff)
                live = mine[:len(want)]
                assert m_lo <= live[:, 0].min() and live[:, 0].max() < m_hi
                assert n_lo <= live[:, 1].min() and live[:, 1].max() < n_hi


def test_xcd_tile_counts_differ_by_at_most_one_block(host_maps):
    """Column order: the XCDs' rectangles differ by at most one panel row of a column set (<= one block of mblock rows)."""
    for (mt, nt, xc, mb, g), (grid, xc_eff, t) in host_maps.items():
        if xc_eff == 1:
            continue
        counts = [int((t[x::8, 0] >= 0).sum()) for x in range(8)]
        assert max(counts) - min(counts) <= mb * (nt // xc_eff), f"{(mt, nt, xc, mb)}: {counts}"
        assert max(counts) - min(counts) <= nt // xc_eff


def test_row_sets_share_a_panels_in_step(host_maps):
    """The XCDs of one row set (they differ in the column set only) are on the SAME A panel at every slot: the second fetch of
    a panel follows the first at once."""
    for (mt, nt, xc, mb, g), (grid, xc_eff, t) in host_maps.items():
        if xc_eff == 1:
            continue
        for rset in range(8 // xc_eff):
            first = t[rset * xc_eff::8, 0]
            for cset in range(1, xc_eff):
                assert np.array_equal(t[rset * xc_eff + cset::8, 0], first)
