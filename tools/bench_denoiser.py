"""What one denoised feature map costs: ViT-B/14 DINOv2 at 518 x 518 (37 x 37 tokens), 32 views, random well-conditioned
weights, a 1-block denoiser.  Four legs, ms per view:
  (a) the bf16 extractor alone                                   HipViT.forward_features
  (b) (a) + the exact-fp32 denoiser forward (the default)        Stage2Engine.forward on the returned features
  (c) (a) + the bf16 denoiser forward on the returned features   dvt_denoiser_forward_bf16
  (d) the fused call, image in, denoised features out            dvt_vit_forward_denoised
The legs are INTERLEAVED in one process (a, b, c, d, a, b, ...: the clock drifts over a run), one sample of each per round,
`reps` rounds after `warmup` rounds; medians are reported, every sample is kept.  Prints one JSON line and, with --out,
writes it to that file.

    python tools/bench_denoiser.py [--views 32] [--reps 20] [--warmup 3] [--out profiles/denoiser/bench_denoiser.json]

Run it under a time limit of its own (`timeout -k 10 300 python tools/...`).
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

from dvt_amd.models import PretrainedViTWrapper  # noqa: E402
from dvt_amd.models.online_denoiser import Denoiser  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--num_blocks", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model, size, g, dim = "vit_base_patch14_dinov2.lvd142m", 518, 37, 768
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = PretrainedViTWrapper(model, stride=14, img_size=(size, size), allow_random_init=True, dtype="bfloat16")
    den = Denoiser(g, g, dim, num_blocks=a.num_blocks, device=dev, seed=0, inference_dtype="bfloat16")
    # O(1) norm affines and biases instead of the trainer's initial ones / zeros (arithmetic cost does not depend on them)
    gen = torch.Generator().manual_seed(1)
    sd = {k: (v.detach().cpu() + 0.2 * torch.randn(v.shape, generator=gen) if v.dim() == 1 else v.detach().cpu())
          for k, v in den.engine.views().items()}
    den.load_state_dict(sd)
    vit, hd, eng = w._engine(dev), den._bf16_for(g, g), den.engine
    x = torch.randn(a.views, 3, size, size, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    feat = torch.empty(a.views, g, g, dim, device=dev)
    out32, out16 = torch.empty(a.views, g * g, dim, device=dev), torch.empty_like(feat)
    fused = {}

    def leg_a():
        vit.forward_features(x, out=feat, max_batch=400)

    def leg_b():
        leg_a()
        eng.forward(feat.view(a.views, g * g, dim), out=out32)

    def leg_c():
        leg_a()
        hd.forward(feat, out=out16)

    def leg_d():
        fused["out"] = hd.forward_fused(vit, x, max_batch=400)[0]

    legs = {"a_extractor": leg_a, "b_plus_fp32_denoiser": leg_b, "c_plus_bf16_denoiser": leg_c, "d_fused": leg_d}
    ms = {k: [] for k in legs}
    for r in range(a.warmup + a.reps):
        for k, fn in legs.items():
            t = timed(fn)
            if r >= a.warmup:
                ms[k].append(t)
    assert torch.equal(fused["out"], out16), "the fused call and the composition disagree"
    assert bool(torch.isfinite(out16).all()) and bool(torch.isfinite(out32).all())
    rel = float((out16.view_as(out32) - out32).norm() / out32.norm())
    med = {k: statistics.median(v) / a.views for k, v in ms.items()}
    row = {"model": model, "weights": "random", "size": size, "grid": [g, g], "views": a.views, "denoiser_blocks": a.num_blocks,
           "reps": a.reps, "warmup": a.warmup, "legs": "interleaved", "ms_per_view": {k: round(v, 5) for k, v in med.items()},
           "b_minus_a": round(med["b_plus_fp32_denoiser"] - med["a_extractor"], 5),
           "c_minus_a": round(med["c_plus_bf16_denoiser"] - med["a_extractor"], 5),
           "d_minus_a": round(med["d_fused"] - med["a_extractor"], 5),
           "bf16_vs_fp32_denoiser_rel_l2": rel,
           "ms_all": {k: [round(t, 3) for t in v] for k, v in ms.items()}}
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
