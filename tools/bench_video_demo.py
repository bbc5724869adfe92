"""Time per frame of the feature-video demo at its shape (ViT-B/14, stride 4, 490 x 854: 120 x 211 tokens): the extractor in
both dtypes with its attention / GEMM split from the in-process probes, everything after the extractor (dvt_amd.video), the
launch count, and the same post-processing written with torch ops on the same GPU.  The two post-processing paths are
interleaved and medians are reported.  Prints one JSON line.

    python tools/bench_video_demo.py [--reps 20] [--extractor_reps 5]

The torch comparison is NOT the same filter: torch has no Pillow-exact 8-bit bicubic, it runs F.interpolate(mode="bicubic")
on float pictures (a = -0.75, no uint8 intermediate), and its colour maps are table gathers from the same 256-entry tables.

The exact-fp32 extractor's kernels carry no probes: its attention / GEMM split is reported as "not probed", never as zeros.
The post-processing legs run on ONE feature tensor (78 MB) that may stay in the 256 MB last-level cache between repetitions, so
their times say nothing about the share of HBM bandwidth the apply pass reaches: not measured here.
Everything runs in this one process, as tools/bench_vis.py does; run it under a time limit of its own (`timeout -k 10 400
python tools/bench_video_demo.py`) so that trouble ends it.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "denoising-vit_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from dvt_amd import _lib  # noqa: E402
from dvt_amd import video as VD  # noqa: E402
from dvt_amd.models import PretrainedViTWrapper  # noqa: E402

H, W, STRIDE, GH, GW, C, K = 490, 854, 4, 120, 211, 768, 8


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def torch_frame(x, M, centers, inferno, rainbow):
    """The script's per-frame lines with torch ops (fp32), all nine pictures at full size."""
    n = x.shape[0]
    P = x @ M
    unit = (P - P.min(0, keepdim=True)[0]) / (P.max(0, keepdim=True)[0] - P.min(0, keepdim=True)[0])
    second = 1 - P[:, 4]
    second_u = (second - second.min()) / (second.max() - second.min())
    mask_fg, mask_std = (second > 0.1)[:, None], (P[:, 6] > 0)[:, None]
    labels = (F.normalize(x, dim=1) @ F.normalize(centers, dim=1).T).argmax(1)
    norm = F.softmax(x.norm(dim=1) / 5, dim=0)
    norm = (norm - norm.min()) / (norm.max() - norm.min())
    lut = lambda v: inferno[(v * 256).long().clamp(0, 255)]  # noqa: E731
    pics = [unit[:, 0:3], unit[:, 3:6], rainbow[labels], lut(unit[:, 3]), lut(second_u), lut(unit[:, 5]),
            unit[:, 7:10] * mask_fg, unit[:, 10:13] * mask_std, lut(norm)]
    tok = (torch.stack(pics).reshape(9, GH, GW, 3) * 255).to(torch.uint8)
    up = F.interpolate(tok.permute(0, 3, 1, 2).float(), size=(H, W), mode="bicubic", align_corners=False)
    return up.clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--extractor_reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"shape": {"image": [H, W], "stride": STRIDE, "grid": [GH, GW], "tokens": 1 + GH * GW, "channels": C}, "reps": a.reps}
    img = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(0)).to(dev)
    feats = None
    # attention FLOPs per frame as the probes count them vs the plain formula 4 S^2 64 heads depth
    S = 1 + GH * GW
    out["flops_formula_tf"] = {"attention": 4 * S * S * 64 * 12 * 12 / 1e12, "gemm": 2 * S * 12 * C * C * 12 / 1e12}
    for dtype in ("bfloat16", "float32"):
        vit = PretrainedViTWrapper("vit_base_patch14_dinov2.lvd142m", stride=STRIDE, img_size=(H, W), allow_random_init=True,
                                   dtype=dtype)
        vit.features_nhwc(img)  # warm-up: code objects, workspace
        vit.features_nhwc(img)
        ms = [once(lambda: vit.features_nhwc(img)) for _ in range(a.extractor_reps)]
        _lib.prof_enable(["vit_gemm", "vit_attn"])
        f = vit.features_nhwc(img)
        torch.cuda.synchronize()
        g, at = _lib.prof_collect("vit_gemm"), _lib.prof_collect("vit_attn")
        _lib.prof_enable([])
        rec = {"ms_per_frame_median": statistics.median(ms), "ms_per_frame_all": ms}
        for name, pr in (("gemm", g), ("attention", at)):
            rec[name] = "not probed" if pr["launches"] == 0 else {
                "ms": pr["total_ms"], "launches": pr["launches"], "work": pr["work"], "tflops": pr["work"] / pr["total_ms"] / 1e9}
        if g["launches"] and at["launches"]:
            rec["attention_share_of_probed_ms"] = at["total_ms"] / (g["total_ms"] + at["total_ms"])
        out[f"extractor_{dtype}"] = rec
        if dtype == "bfloat16":
            feats = f.clone()
        del vit
        torch.cuda.empty_cache()
    # ---- everything after the extractor
    rng = np.random.RandomState(0)
    stats = {"reduct_mat_full": (rng.standard_normal((C, 3)) / np.sqrt(C)).astype(np.float32),
             "standard_mapping": (rng.standard_normal((C, 1)) / np.sqrt(C)).astype(np.float32)}
    eng = VD.VideoDemoEngine(dev, (GH, GW), C, (H, W), stats, num_clusters=K, seed=0)
    out["fit_ms_frame0"] = once(lambda: eng.fit(feats))
    out["fit_ms_frame0_second_call"] = once(lambda: eng.fit(feats))
    before = eng.launches
    eng.frame(feats, image=img)
    out["launches_per_frame"] = eng.launches - before
    x = feats.reshape(-1, C)
    inferno = torch.from_numpy(VD.color_table_u8("inferno")).to(dev).float() / 255
    rainbow = torch.from_numpy(VD.label_table_u8("rainbow", K)).to(dev).float() / 255
    for _ in range(3):
        eng.frame(feats, image=img)
        torch_frame(x, eng.M, eng.centers, inferno, rainbow)
    hip, tor = [], []
    for _ in range(a.reps):  # interleaved
        hip.append(once(lambda: eng.frame(feats, image=img)))
        tor.append(once(lambda: torch_frame(x, eng.M, eng.centers, inferno, rainbow)))
    out["post_ms_per_frame"] = {"hip_median": statistics.median(hip), "hip_min": min(hip), "hip_max": max(hip),
                                "torch_median": statistics.median(tor), "torch_min": min(tor), "torch_max": max(tor),
                                "note": "torch: F.interpolate bicubic on float pictures, not Pillow's 8-bit filter; no input picture"}
    host = torch.empty(eng.full.shape, dtype=torch.uint8, pin_memory=True)
    out["copy_out_ms"] = statistics.median([once(lambda: host.copy_(eng.full, non_blocking=True)) for _ in range(5)])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
