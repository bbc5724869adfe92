"""Developer tool (product library): the tile-order and cache-policy knobs of the 256 x 256 bf16 GEMM at the bench's launch
size, per GEMM type, as an interleaved A/B inside one process -- every variant is timed once per round, the rounds alternate
the variants, the first round is dropped.  The first row of every table is the setting of rounds 2-6 spelled out (M blocks of 4
for qkv / fc1 and of 1 for proj / fc2, one column set, no policy); mblock 0 / xcols 0 / policy 128 (auto: mask 47 on these shapes) are the library's defaults.

    python tools/bench_vit_xcols.py [views] [out.json]

Knobs: W KiB per N-tile group (dvt_tune_set(1, KiB)) x M panels per block (-100 - b) x XCD column sets (-70 - x) x epilogue
cache policy (-200000 - mask; include/dvt_hip.h).  The last section runs the whole extractor under a few settings.
"""
import ctypes as C
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "denoising-vit_amd")]
from dvt_amd import _lib  # noqa: E402
import dvt_amd.vit  # noqa: E402,F401  (registers the signatures)

VIEWS = int(sys.argv[1]) if len(sys.argv) > 1 else 396
OUT = sys.argv[2] if len(sys.argv) > 2 else None
S_PAD, DIM, HID, HEADS = 1376, 768, 3072, 12
M = (VIEWS * S_PAD + 255) // 256 * 256
dev = torch.device("cuda:0")
L = _lib.lib()
ROUNDS, REPS = 5, 3
XCOLS_AUTO_KIB = int(os.environ.get("DVT_XCOLS_KIB", "2400"))  # "xcols auto" below: at most this much W per XCD
assert L.dvt_tune_set(1, -100000 - XCOLS_AUTO_KIB) == 0


def stream():
    return torch.cuda.current_stream().cuda_stream


def knobs(kib, mblock, xcols, policy):
    assert L.dvt_tune_set(1, kib) == 0 and L.dvt_tune_set(1, -100 - mblock) == 0
    assert L.dvt_tune_set(1, -70 - xcols) == 0 and L.dvt_tune_set(1, -200000 - policy) == 0


def defaults():
    knobs(4800, 0, 0, 128)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def sweep(name, fn, variants, flops, nk, tiles):
    res = {v: [] for v in variants}
    for rnd in range(ROUNDS):
        for v in variants:
            knobs(*v)
            t = timed(fn)
            if rnd:
                res[v].append(t)
    defaults()
    rounds_of_tiles = -(-tiles // 256)
    rows = []
    print(f"== {name}: M {M}, {tiles} tiles, {nk} k-tiles; median of {ROUNDS - 1} rounds x {REPS} launches")
    base = sorted(res[variants[0]])[len(res[variants[0]]) // 2]
    for v in variants:
        ts = sorted(res[v])
        med = ts[len(ts) // 2]
        rows.append({"group_kib": v[0], "mblock": v[1], "xcols": v[2], "policy": v[3], "ms": med, "min_ms": ts[0], "max_ms": ts[-1],
                     "tflops": flops / med * 1e-9, "ktile_us": med * 1e3 / (rounds_of_tiles * nk)})
        print(f"group {v[0]:5d} KiB mblock {v[1]:2d} xcols {v[2]} policy {v[3]:3d}: {med:7.3f} ms (min {ts[0]:7.3f} max {ts[-1]:7.3f}) "
              f"{flops / med * 1e-9:7.1f} TF/s  k-tile {med * 1e3 / (rounds_of_tiles * nk):5.3f} us  {100 * (base / med - 1):+5.1f} %",
              flush=True)
    return rows


g = torch.Generator(device=dev).manual_seed(0)
xb = (torch.randn(M, DIM, generator=g, device=dev)).bfloat16()
stats = torch.stack([torch.zeros(M, device=dev), torch.ones(M, device=dev)], 1).contiguous()
doc = {"views": VIEWS, "M": M, "gemms": {}}

# ---- qkv: N 2304 (9 N tiles: no equal column sets), K 768
w = (torch.randn(3 * DIM, DIM, generator=g, device=dev) * 0.05).bfloat16()
b = torch.zeros(3 * DIM, device=dev)
cs = w.float().sum(1).contiguous()
qk = torch.empty(M, 2 * DIM, device=dev, dtype=torch.bfloat16)
vt = torch.empty(VIEWS + 1, HEADS, 64, S_PAD, device=dev, dtype=torch.bfloat16)
var = [(4800, mb, 1, pol) for mb in (4, 1, 2, 8, 16, 32, 64, 0) for pol in (0, 16)] + [(2400, 4, 1, 0), (1200, 4, 1, 0)]
doc["gemms"]["qkv"] = sweep("qkv", lambda: L.dvt_vit_gemm_qkv(xb.data_ptr(), w.data_ptr(), b.data_ptr(), qk.data_ptr(), vt.data_ptr(),
                                                              M, DIM, HEADS, S_PAD, VIEWS, stats.data_ptr(), cs.data_ptr(), 0.18, stream()),
                            var, 2.0 * M * 3 * DIM * DIM, DIM // 64, (M // 256) * 9)
del qk, vt

# ---- fc1: N 3072 (12 N tiles), K 768
w = (torch.randn(HID, DIM, generator=g, device=dev) * 0.05).bfloat16()
b = torch.zeros(HID, device=dev)
cs = w.float().sum(1).contiguous()
hid = torch.empty(M, HID, device=dev, dtype=torch.bfloat16)
var = [(4800, mb, xc, pol) for xc in (1, 2) for mb in (4, 1, 2, 8, 16, 32, 0) for pol in (0, 40)]
var += [(4800, mb, 4, pol) for mb in (4, 8) for pol in (0, 40)]
var += [(4800, 4, xc, 8) for xc in (1, 2)] + [(2400, 4, 1, 0), (4800, 0, 0, 128)]
doc["gemms"]["fc1"] = sweep("fc1", lambda: L.dvt_vit_gemm_lnfold(xb.data_ptr(), w.data_ptr(), b.data_ptr(), hid.data_ptr(), M, HID, DIM,
                                                                 stats.data_ptr(), cs.data_ptr(), 1, stream()),
                            var, 2.0 * M * HID * DIM, DIM // 64, (M // 256) * 12)

# ---- proj (K 768) and fc2 (K 3072): N 768 (3 N tiles), the residual epilogue with its LayerNorm producer side
x = torch.zeros(M, DIM, device=dev)
xo = torch.empty(M, DIM, device=dev, dtype=torch.bfloat16)
st = torch.empty(M, 2, device=dev)
part = torch.empty(DIM // 64, M, 2, device=dev)
gm = torch.full((DIM,), 1e-3, device=dev)
b = torch.zeros(DIM, device=dev)
RES_VAR = [(4800, mb, 1, p) for mb in (1, 2, 4, 8, 16) for p in (0, 1, 2, 2 | 64, 4, 7, 7 | 64)] + [(4800, 0, 0, 128)]
for name, a_op, k in (("proj", xb, DIM), ("fc2", hid, HID)):
    w = (torch.randn(DIM, k, generator=g, device=dev) * 0.02).bfloat16()
    doc["gemms"][name] = sweep(name, lambda: L.dvt_vit_gemm_residual_stats(a_op.data_ptr(), w.data_ptr(), b.data_ptr(), gm.data_ptr(),
                                                                           x.data_ptr(), xo.data_ptr(), st.data_ptr(), part.data_ptr(),
                                                                           M, DIM, k, C.c_float(1e-6), stream()),
                               RES_VAR, 2.0 * M * DIM * k, k // 64, (M // 256) * 3)
del x, xo, hid, xb

# ---- the whole extractor (one launch of VIEWS views) under the settings that matter
from dvt_amd.models import PretrainedViTWrapper  # noqa: E402

with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    vit = PretrainedViTWrapper("vit_base_patch14_dinov2.lvd142m", stride=14, allow_random_init=True)
img = torch.randn(VIEWS, 3, 518, 518, device=dev)
out = torch.empty(VIEWS, 37, 37, 768, device=dev)
vit.features_nhwc(img, out=out, max_batch=VIEWS + 2)
EXT = [("one column set, no policy", -71, 0), ("xcols auto", -70, 0), ("xcols 2 forced", -72, 0), ("xcols 4 forced", -74, 0),
       ("xcols auto + hid sc1", -70, 40), ("xcols auto + residual sc1 stores", -70, 2 | 64),
       ("xcols auto + every policy, sc1", -70, 127), ("xcols auto + every policy, nt", -70, 31),
       ("one column set + mask 47", -71, 47), ("xcols auto + mask 47", -70, 47), ("library defaults", -70, 128)]
res = {e: [] for e in EXT}
for rnd in range(4):
    for e in EXT:
        L.dvt_tune_set(1, e[1])
        L.dvt_tune_set(1, -200000 - e[2])
        t = timed(lambda: vit.features_nhwc(img, out=out, max_batch=VIEWS + 2))
        if rnd:
            res[e].append(t)
defaults()
print(f"== extractor, {VIEWS} views, one launch")
doc["extractor"] = []
for e in EXT:
    ts = sorted(res[e])
    doc["extractor"].append({"setting": e[0], "ms": ts[1], "min_ms": ts[0], "max_ms": ts[-1]})
    print(f"{e[0]:40s}: {ts[1]:8.2f} ms (min {ts[0]:8.2f} max {ts[-1]:8.2f})")
if OUT:
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
