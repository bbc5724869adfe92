"""The DINO / DeiT-III / AugReg patch-8 / patch-16 backbones on the HIP extractor, random weights: ms per view in bf16 and in
exact fp32, at the model's native size (stride = patch) and at 518 x 518 padded down to a multiple of the patch (512 x 512;
stride = patch), full depth.  ViT-B/14 DINOv2 at 518 x 518 is measured beside them as the yardstick.  Prints one JSON line
per model and, with --out, writes them to that file.

    python tools/bench_backbones.py [--views 32] [--views_f32 8] [--reps 5] [--out profiles/backbones/bench_backbones.jsonl]

Timing: `reps` samples of one features_nhwc call over all views between two device events, after one warm-up call; the
median is reported, every sample is kept.  FLOP per view (algorithmic, multiply-add = 2): depth * (2 S dim * 12 dim + 4 S^2
dim) + the patch embedding, S = tokens.  Run it under a time limit of its own (`timeout -k 10 500 python tools/...`).
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

from dvt_amd import vit as V  # noqa: E402
from dvt_amd.models import PretrainedViTWrapper  # noqa: E402

MODELS = ["vit_small_patch16_224.dino", "vit_small_patch8_224.dino", "vit_base_patch16_224.dino", "vit_base_patch8_224.dino",
          "deit3_base_patch16_224.fb_in1k", "vit_base_patch16_384.augreg_in21k_ft_in1k", "vit_base_patch14_dinov2.lvd142m"]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(model, size, views, dtype, reps, dev):
    spec = V.SPECS[model]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = PretrainedViTWrapper(model, stride=spec.patch, img_size=(size, size), allow_random_init=True, dtype=dtype)
    g = size // spec.patch
    tok = 1 + spec.n_reg + g * g
    x = torch.randn(views, 3, size, size, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    feat = torch.empty(views, g, g, spec.dim, device=dev)
    run = lambda: w.features_nhwc(x, out=feat, max_batch=400)  # noqa: E731
    run()
    ms = [timed(run) for _ in range(reps)]
    med = statistics.median(ms)
    flop = spec.depth * (2 * tok * spec.dim * 12 * spec.dim + 4 * tok * tok * spec.dim) + 2 * g * g * 3 * spec.patch ** 2 * spec.dim
    assert bool(torch.isfinite(feat).all())
    return {"size": size, "tokens": tok, "s_pad": int(w._engine(dev).cfg.s_pad), "views": views,
            "ms_per_view": med / views, "tflops": flop * views / (med * 1e-3) / 1e12, "gflop_per_view": flop / 1e9,
            "ms_all": [round(v, 3) for v in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=32, help="views per bf16 sample")
    ap.add_argument("--views_f32", type=int, default=8, help="views per fp32 sample")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--models", nargs="*", default=MODELS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for model in a.models:
        spec = V.SPECS[model]
        sizes = {"native": spec.img_size, "518": 518 // spec.patch * spec.patch}
        row = {"model": model, "weights": "random", "dim": spec.dim, "depth": spec.depth, "patch": spec.patch, "reps": a.reps}
        for dtype, key, views in (("bfloat16", "bf16", a.views), ("float32", "fp32", a.views_f32)):
            for name, size in sizes.items():
                if name == "518" and size == spec.img_size:
                    row[f"{key}_518"] = row[f"{key}_native"]
                    continue
                row[f"{key}_{name}"] = measure(model, size, views, dtype, a.reps, dev)
                torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        lines.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
