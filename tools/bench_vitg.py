"""ViT-g/14 (dim 1536, 40 blocks, SwiGLU 4096) at 518 x 518 on the bf16 extractor, random weights: ms per view and TF/s, and an
interleaved A/B of the SwiGLU fc1 in one process -- FUSED (dvt_vit_gemm_swiglu: packed weights, silu(gate) * value in the
epilogue, a half-width [T, 4096] store; plain and LayerNorm-folded) against UNFUSED (the bias epilogue to a full-width
[T, 8192] + dvt_vit_swiglu_act).  Prints one JSON line.

    python tools/bench_vitg.py [--views 64] [--reps 5] [--ab_views 64] [--ab_reps 15] [--ab_launches 10]

FLOP count used (algorithmic, per view, 1370 tokens, multiply-add = 2): per block 2 * 1370 * 1536 * (3 * 1536 + 1536 + 8192 +
4096) = 7.76e10 in the linear layers + 4 * 1370^2 * 1536 = 1.15e10 in the attention; 40 blocks + the patch embedding
(2 * 1369 * 588 * 1536) = 3.57 TFLOP per view.
Run it under a time limit of its own (`timeout -k 10 500 python tools/bench_vitg.py`).
"""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "denoising-vit_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from dvt_amd import _lib  # noqa: E402
from dvt_amd import vit as V  # noqa: E402
from dvt_amd.models import PretrainedViTWrapper  # noqa: E402

DIM, DEPTH, HID, TOK = 1536, 40, 4096, 1370
FLOP_VIEW = DEPTH * (2 * TOK * DIM * (3 * DIM + DIM + 2 * HID + HID) + 4 * TOK * TOK * DIM) + 2 * 1369 * 588 * DIM


def timed(fn, n=1):
    """ms per call of `fn`: n back-to-back calls between two device events (no host wait inside the bracket)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ab_views", type=int, default=64)
    ap.add_argument("--ab_reps", type=int, default=15)
    ap.add_argument("--ab_launches", type=int, default=10, help="launches per timed sample of an A/B leg")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    s = _lib.stream
    out = {"model": "vit_giant_patch14_dinov2.lvd142m", "dtype": "bf16", "weights": "random", "image": 518, "tokens": TOK,
           "tflop_per_view": FLOP_VIEW / 1e12, "views": a.views, "reps": a.reps}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = PretrainedViTWrapper("vit_giant_patch14_dinov2.lvd142m", stride=14, allow_random_init=True)
    x = torch.randn(a.views, 3, 518, 518, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    feat = torch.empty(a.views, 37, 37, DIM, device=dev)
    run = lambda: w.features_nhwc(x, out=feat, max_batch=400)  # noqa: E731
    run()
    ms = [timed(run) for _ in range(a.reps)]
    med = statistics.median(ms)
    out.update(ms_per_view=med / a.views, tflops=FLOP_VIEW * a.views / (med * 1e-3) / 1e12, ms_all=[round(v, 2) for v in ms],
               launch_plan=w._engine(dev).launch_plan(a.views, 400))
    del w, x, feat
    torch.cuda.empty_cache()

    # ---- the SwiGLU fc1 alone, at the extractor's shape: T rows of `ab_views` views (s_pad 1376, whole 256-row tiles)
    T = (a.ab_views * 1376 + 255) // 256 * 256
    g = torch.Generator(device=dev).manual_seed(1)
    xa = torch.randn(T, DIM, generator=g, device=dev).bfloat16()
    W = (torch.randn(2 * HID, DIM, generator=g, device=dev) / DIM ** 0.5).bfloat16()
    b = torch.randn(2 * HID, generator=g, device=dev) * 0.2
    Wp, bp = V.swiglu_pack(W).contiguous(), V.swiglu_pack(b).contiguous()
    cs = Wp.float().sum(1).contiguous()
    st = torch.stack([torch.zeros(T, device=dev), torch.ones(T, device=dev)], 1).contiguous()
    full = torch.empty(T, 2 * HID, device=dev, dtype=torch.bfloat16)
    hid_u = torch.empty(T, HID, device=dev, dtype=torch.bfloat16)
    hid_f = torch.empty(T, HID, device=dev, dtype=torch.bfloat16)
    hid_l = torch.empty(T, HID, device=dev, dtype=torch.bfloat16)

    def fused():
        _lib.check(L.dvt_vit_gemm_swiglu(xa.data_ptr(), Wp.data_ptr(), bp.data_ptr(), hid_f.data_ptr(), T, HID, DIM, None, None,
                                         s()), "gemm_swiglu")

    def fused_fold():
        _lib.check(L.dvt_vit_gemm_swiglu(xa.data_ptr(), Wp.data_ptr(), bp.data_ptr(), hid_l.data_ptr(), T, HID, DIM,
                                         st.data_ptr(), cs.data_ptr(), s()), "gemm_swiglu folded")

    def unfused():
        _lib.check(L.dvt_vit_gemm_bias(xa.data_ptr(), W.data_ptr(), b.data_ptr(), full.data_ptr(), T, 2 * HID, DIM, s()), "gemm_bias")
        _lib.check(L.dvt_vit_swiglu_act(full.data_ptr(), hid_u.data_ptr(), T, HID, s()), "swiglu_act")

    legs = {"fused": fused, "fused_lnfold": fused_fold, "unfused": unfused}
    for fn in legs.values():
        fn()
    times = {k: [] for k in legs}
    for _ in range(a.ab_reps):  # interleaved: every repetition times every leg once (ab_launches calls between device events)
        for k, fn in legs.items():
            times[k].append(timed(fn, a.ab_launches))
    flop = 2.0 * T * 2 * HID * DIM
    ab = {k: {"ms_median": statistics.median(v), "ms_min": min(v), "tflops_median": flop / (statistics.median(v) * 1e-3) / 1e12}
          for k, v in times.items()}
    # (mean 0, rstd 1: the folded leg computes the plain product; the unfused leg rounds g and v to bf16 before the product)
    d = (hid_f.float() - hid_u.float()).abs().max().item()
    ab["rows"], ab["reps"], ab["views"], ab["launches_per_sample"] = T, a.ab_reps, a.ab_views, a.ab_launches
    ab["max_abs_diff_fused_vs_unfused"] = d
    ab["fused_equals_folded_bits"] = bool(torch.equal(hid_f, hid_l))
    ab["fused_over_unfused"] = ab["fused"]["ms_median"] / ab["unfused"]["ms_median"]
    ab["bytes_not_moved_per_block_at_385_views"] = 2 * 385 * 1376 * 2 * HID * 2
    out["swiglu_fc1_ab"] = ab
    print(json.dumps(out))


if __name__ == "__main__":
    main()
