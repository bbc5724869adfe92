"""Time the linear-probe segmentation evaluation (csrc/dvt_seg.hip): the head's training step alone, the frozen ViT-B/14
forward it sits behind, and slide inference of one 512 x 683 image (two 512 x 512 crops), with random ViT weights.

Prints one JSON line.  Train iterations/s count the backbone forward of the batch, the head step and AdamW; the data
pipeline (host decode and augmentation) is not part of this port, so no host-feed time is measured.

    python tools/bench_seg_eval.py [--classes 21 --steps 20 --warmup 3 --dtype bfloat16]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "denoising-vit_amd"))

import torch  # noqa: E402

from dvt_amd.seg import SegHeadEngine, ViTBackbone  # noqa: E402
from dvt_amd.vit import random_state_dict  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--classes", type=int, default=21)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float32"])
    a = p.parse_args()
    dev = torch.device("cuda:0")
    C = 768
    sd = random_state_dict(C, 12, 14, 1 + 37 * 37, seed=0, well_conditioned=True)
    bb = ViTBackbone(sd, 14, dev, dtype=a.dtype)
    eng = SegHeadEngine(C, a.classes, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    res = {"box": torch.cuda.get_device_name(0), "classes": a.classes, "dtype": a.dtype}
    for B in (2, 16):
        img = torch.randn(B, 3, 512, 512, device=dev, generator=g)
        lab = torch.randint(0, a.classes, (B, 512, 512), device=dev, generator=g).to(torch.uint8)
        feats = bb(img)
        t_bb = timed(lambda: bb(img), a.steps, a.warmup)

        def head():
            eng.train_step(feats, lab)
            eng.adamw_step(1e-3, 1e-4)

        t_head = timed(head, a.steps, a.warmup)

        def it():
            f = bb(img)
            eng.train_step(f, lab)
            eng.adamw_step(1e-3, 1e-4)

        t_it = timed(it, a.steps, a.warmup)
        res[f"b{B}"] = {"train_it_per_s": 1.0 / t_it, "iter_ms": 1e3 * t_it, "backbone_ms": 1e3 * t_bb,
                        "head_step_ms": 1e3 * t_head, "head_fraction_of_backbone": t_head / t_bb,
                        "host_feed_wait_ms": None}
    img = torch.randn(3, 512, 683, device=dev, generator=g)
    label = torch.randint(0, a.classes, (512, 683), device=dev, generator=g).to(torch.uint8)
    hist = torch.zeros(3, a.classes, dtype=torch.int64, device=dev)
    t_slide = timed(lambda: eng.evaluate_image(img, label, hist, bb), a.steps, a.warmup)
    res["slide_512x683_img_per_s"] = 1.0 / t_slide
    print(json.dumps(res))


if __name__ == "__main__":
    main()
