"""Time the linear-probe depth evaluation (csrc/dvt_depth.hip): the head's training step (step, clipping, AdamW) at the
NYU training geometry -- batch 2, 30 x 39 tokens, C = 768, labels 416 x 544 -- next to the frozen ViT-B/14 forward of the
same batch (420 x 546 after the centre padding), and the test of one 480 x 640 image (the image and its flip through the
backbone, the head and the metric kernels), with random ViT weights.

Prints one JSON line.

    python tools/bench_depth_eval.py [--steps 20 --warmup 3 --dtype bfloat16]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "denoising-vit_amd"))

import torch  # noqa: E402

from dvt_amd.depth import DepthHeadEngine  # noqa: E402
from dvt_amd.seg import ViTBackbone  # noqa: E402
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
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float32"])
    a = p.parse_args()
    dev = torch.device("cuda:0")
    C, B = 768, 2
    sd = random_state_dict(C, 12, 14, 1 + 37 * 37, seed=0, well_conditioned=True)
    bb = ViTBackbone(sd, 14, dev, dtype=a.dtype, return_cls=True)
    eng = DepthHeadEngine(C, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    img = torch.randn(B, 3, 416, 544, device=dev, generator=g)
    gt = 0.5 + 8 * torch.rand(B, 416, 544, device=dev, generator=g)
    feats, cls = bb(img)
    assert tuple(feats.shape) == (B, 30, 39, C)
    t_bb = timed(lambda: bb(img), a.steps, a.warmup)

    def head():
        eng.train_step(feats, cls, gt, 1000)
        eng.clip_grad_norm(35.0)
        eng.adamw_step(5e-3, 0.01)

    t_head = timed(head, a.steps, a.warmup)
    t_step = timed(lambda: eng.train_step(feats, cls, gt, 1000), a.steps, a.warmup)

    def it():
        f, c = bb(img)
        eng.train_step(f, c, gt, 1000)
        eng.clip_grad_norm(35.0)
        eng.adamw_step(5e-3, 0.01)

    t_it = timed(it, a.steps, a.warmup)
    test_img = torch.randn(3, 480, 640, device=dev, generator=g)
    test_gt = 0.5 + 8 * torch.rand(480, 640, device=dev, generator=g)
    row = torch.zeros(9, device=dev, dtype=torch.float64)
    t_test = timed(lambda: eng.evaluate_image(test_img, test_gt, row, bb), a.steps, a.warmup)
    print(json.dumps({"box": torch.cuda.get_device_name(0), "dtype": a.dtype, "batch": B, "train_it_per_s": 1.0 / t_it,
                      "iter_ms": 1e3 * t_it, "backbone_ms": 1e3 * t_bb, "head_step_clip_adamw_ms": 1e3 * t_head,
                      "head_train_step_ms": 1e3 * t_step, "head_launches": {"train_step": 10 if B < 3 else 11, "clip": 3, "adamw": 1},
                      "head_fraction_of_backbone": t_head / t_bb, "test_480x640_img_per_s": 1.0 / t_test,
                      "test_image_ms": 1e3 * t_test}))


if __name__ == "__main__":
    main()
