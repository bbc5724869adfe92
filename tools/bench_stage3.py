"""Time the stage-3 student step (csrc/dvt_stage3.hip): forward + loss + backward + AdamW of a whole ViT, in exact fp32 or
in the opt-in bf16 mode (`--dtype bfloat16`: bf16 operands in the forward and data-gradient GEMMs of the linear layers), with
`--attention bfloat16` on top of it the bf16 flash attention (no probabilities kept) and with `--weight_grad bfloat16` the bf16
split-K weight gradients.

Prints one JSON line: ms per step, images/s, and the step's matrix FLOPs per second against the 157 TF/s fp32 MFMA peak
of the MI355X.  The FLOPs count the student only (forward 1x, backward 2x; tokens padded to s_pad rows as the kernels
run them, attention over all s_pad keys); the teacher's forward (fp32 ViT + the denoiser block, about 1/3 of the
student's step) is not part of the timed step.

    python tools/bench_stage3.py [--dim 768 --depth 12 --img 518 --batch 64 --steps 3 --warmup 1]
                                 [--input_size H W] [--stride_size S] [--pos_grid G0]
                                 [--dtype float32|bfloat16] [--attention float32|bfloat16] [--weight_grad float32|bfloat16] [--ab N]
                                 [--teacher none|float32|bfloat16]

`--teacher float32|bfloat16` (default none: the student alone, the output as it always was): a stage-3 ITERATION -- the
teacher's forward (`Denoiser` over a `PretrainedViTWrapper` of that dtype with random weights, as `stage3.build_models` builds
it for --teacher_dtype) producing the target, then the student's step against it.  With `--ab` every leg's timed unit is
teacher + student, the teacher timed on its own inside it; the JSON line gains `teacher_ms` (median, min, max over all timed
iterations) and per leg `iteration_ms`.  Without `--ab` it gains `teacher_ms` and `iteration_ms` of the one mode.  Needs the
ViT-B/14 or ViT-S/14 geometry (`--dim 768 --depth 12` or `--dim 384 --depth 12`) at stride 14 without --pos_grid.

`--ab N`: an interleaved A/B of the three arithmetics in one process on one engine -- fp32 step, bf16 step, bf16 step with
bf16 attention, fp32 step, ... N of each after the warm-up of all, every step timed on its own (device synchronised on both
sides).  The clock of the chip
drifts over a run, so two runs one after the other do not compare; alternating steps see the same clock.  The JSON line then
carries per leg the median, minimum and maximum ms per step and the workspace bytes per image of its mode (the increment of
the workspace from one image to two), `bf16_faster_than_fp32_spread`: whether the bf16 median lies below the fp32 median by
more than the fp32 leg's own min-max spread, and `bf16_attn_faster_than_bf16_spread`: the same for the attention leg against
the bf16 leg.  A fourth leg, `bfloat16_attn_wgrad` (gemm_mode 7: the attention leg plus the bf16 weight gradients), is interleaved
with the others; `wgrad_faster_than_bf16_attn_spread` compares it with the attention leg in the same way.  All legs run the same slicing: the one the largest workspace (bf16, fp32 attention) allows.

`--input_size` / `--stride_size` set another geometry than `--img` square at stride 14; `--pos_grid G0` keeps the position
table at G0 x G0 (37 for the DINOv2 checkpoints) and resamples it to the run's grid in every step, e.g.
    --input_size 224 224 --pos_grid 37                     (16 x 16 tokens)
    --stride_size 7 --pos_grid 37 --micro_batch 1          (73 x 73 tokens)
The resample's launches are not matrix work and are not in the FLOPs; the JSON line names the grid and the table.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "denoising-vit_amd"))

import torch  # noqa: E402

from dvt_amd import s3  # noqa: E402
from dvt_amd.vit import random_state_dict  # noqa: E402

PEAK_FP32 = 157e12


def step_flops(cfg, batch):
    R, C, F, Tp = batch * cfg.s_pad, cfg.dim, cfg.mlp_dim, cfg.s_pad
    patch = 2 * R * C * cfg.k_patch
    block = 2 * R * C * (3 * C + C + 2 * F) + 2 * 2 * batch * cfg.heads * Tp * Tp * 64
    return 3 * (patch + cfg.depth * block) - 2 * R * C * cfg.k_patch  # no data gradient for the image


def build_teacher(a, cfg, H, W, dev):
    """`Denoiser` over a `PretrainedViTWrapper` with random weights, as stage3.build_models builds the teacher."""
    import warnings
    from dvt_amd.models import Denoiser, PretrainedViTWrapper
    from dvt_amd.vit import SPECS
    name = {768: "vit_base_patch14_dinov2.lvd142m", 384: "vit_small_patch14_dinov2.lvd142m"}.get(a.dim)
    if name is None or SPECS[name].depth != a.depth or a.pos_grid is not None:
        raise SystemExit("--teacher needs --dim 768 or 384 with --depth 12 and no --pos_grid")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vit = PretrainedViTWrapper(name, stride=a.stride_size, img_size=(H, W), allow_random_init=True, dtype=a.teacher)
    kw = {"inference_dtype": "bfloat16"} if a.teacher == "bfloat16" else {}
    return Denoiser(cfg.grid_h, cfg.grid_w, feat_dim=a.dim, vit=vit, num_blocks=1, device=dev, seed=0, **kw)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--depth", type=int, default=12)
    p.add_argument("--img", type=int, default=518)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--micro_batch", type=int, default=0)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--input_size", type=int, nargs=2, default=None, metavar=("H", "W"), help="default: --img square")
    p.add_argument("--stride_size", type=int, default=14)
    p.add_argument("--dtype", default="float32", choices=["float32", "bfloat16"])
    p.add_argument("--attention", default="float32", choices=["float32", "bfloat16"], help="bfloat16 needs --dtype bfloat16")
    p.add_argument("--weight_grad", default="float32", choices=["float32", "bfloat16"], help="bfloat16 needs --dtype bfloat16")
    p.add_argument("--ab", type=int, default=0, metavar="N",
                   help="interleaved fp32 / bf16 / bf16 + bf16 attention A/B, N timed steps of each")
    p.add_argument("--teacher", default="none", choices=["none", "float32", "bfloat16"],
                   help="time the teacher's forward of that dtype in front of every student step (an iteration)")
    p.add_argument("--pos_grid", type=int, default=None,
                   help="grid of the position table when it is not the run's (resampled in every step); default: the run's")
    a = p.parse_args()
    dev = torch.device("cuda:0")
    H, W = a.input_size or (a.img, a.img)
    cfg = s3.make_config(a.dim, a.depth, 14, a.stride_size, H, W)
    eng = s3.Stage3Engine(cfg, dev, pos_grid=a.pos_grid, dtype=a.dtype, attention=a.attention, weight_grad=a.weight_grad)
    n_pos = cfg.grid_h * cfg.grid_w if a.pos_grid is None else a.pos_grid ** 2
    eng.load_timm(random_state_dict(a.dim, a.depth, 14, 1 + n_pos, well_conditioned=True))
    g = torch.Generator(device=dev).manual_seed(0)
    img = torch.randn(a.batch, 3, H, W, device=dev, generator=g)
    tgt = torch.randn(a.batch, cfg.grid_h, cfg.grid_w, a.dim, device=dev, generator=g)
    mb = a.micro_batch or None
    fl = step_flops(cfg, a.batch)
    teacher = build_teacher(a, cfg, H, W, dev) if a.teacher != "none" else None
    t_ms = []

    def target(timed):
        """The iteration's target: the teacher's denoised features (its forward timed on its own), or the random one."""
        if teacher is None:
            return tgt
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            out = teacher(img, return_dict=True)["denoised_feats"].contiguous()
        torch.cuda.synchronize()
        if timed:
            t_ms.append((time.perf_counter() - t0) * 1e3)
        return out

    def stats(v):
        v = sorted(v)
        med = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
        return {"median_ms": round(med, 2), "min_ms": round(v[0], 2), "max_ms": round(v[-1], 2)}
    head = {"bench": "stage3_student_step", "dim": a.dim, "depth": a.depth, "img": a.img if a.input_size is None else [H, W],
            "stride": a.stride_size, "grid": [cfg.grid_h, cfg.grid_w], "pos_grid": a.pos_grid, "batch": a.batch}
    if a.ab > 0:
        if mb is None:  # one slicing for both legs: what the larger (bf16) workspace allows
            eng.set_dtype("bfloat16")
            mb = eng.slice_size(a.batch)
        modes = {"float32": ("float32", "float32"), "bfloat16": ("bfloat16", "float32"),
                 "bfloat16_attn": ("bfloat16", "bfloat16"), "bfloat16_attn_wgrad": ("bfloat16", "bfloat16", "bfloat16")}
        ms = {name: [] for name in modes}
        it_ms = {name: [] for name in modes}
        per_image = {}
        for name, mode in modes.items():
            eng.set_dtype(*mode)
            per_image[name] = eng.workspace_bytes(2) - eng.workspace_bytes(1)
        for i in range(a.warmup + a.ab):
            for dtype, mode in modes.items():
                eng.set_dtype(*mode)
                torch.cuda.synchronize()
                t_it = time.perf_counter()
                tg = target(i >= a.warmup)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loss = eng.train_step(img, tg, micro_batch=mb)
                eng.adamw_step(1e-5, 1e-5)
                torch.cuda.synchronize()
                if i >= a.warmup:
                    ms[dtype].append((time.perf_counter() - t0) * 1e3)
                    it_ms[dtype].append((time.perf_counter() - t_it) * 1e3)
        legs = {}
        for dtype, v in ms.items():
            v = sorted(v)
            med = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
            legs[dtype] = {"median_ms": round(med, 2), "min_ms": round(v[0], 2), "max_ms": round(v[-1], 2),
                           "images_per_s": round(a.batch / med * 1e3, 2), "tflops": round(fl / med / 1e9, 2),
                           "workspace_bytes_per_image": per_image[dtype]}
            if teacher is not None:
                legs[dtype]["iteration_ms"] = stats(it_ms[dtype])
        if teacher is not None:
            head = {**head, "teacher": a.teacher, "teacher_ms": stats(t_ms)}
        f32, b16, att, wg = legs["float32"], legs["bfloat16"], legs["bfloat16_attn"], legs["bfloat16_attn_wgrad"]
        print(json.dumps({**head, "mode": "interleaved_ab", "steps_each": a.ab, "slice": mb, "tflop_per_step": round(fl / 1e12, 2),
                          "float32": f32, "bfloat16": b16, "bfloat16_attn": att, "bfloat16_attn_wgrad": wg,
                          "wgrad_speedup_over_bf16_attn": round(att["median_ms"] / wg["median_ms"], 3),
                          "bf16_attn_spread_ms": round(att["max_ms"] - att["min_ms"], 2),
                          "wgrad_faster_than_bf16_attn_spread":
                              bool(att["median_ms"] - wg["median_ms"] > att["max_ms"] - att["min_ms"]),
                          "speedup": round(f32["median_ms"] / b16["median_ms"], 3),
                          "attn_speedup_over_bf16": round(b16["median_ms"] / att["median_ms"], 3),
                          "bf16_spread_ms": round(b16["max_ms"] - b16["min_ms"], 2),
                          "bf16_attn_faster_than_bf16_spread":
                              bool(b16["median_ms"] - att["median_ms"] > b16["max_ms"] - b16["min_ms"]),
                          "fp32_spread_ms": round(f32["max_ms"] - f32["min_ms"], 2),
                          "bf16_faster_than_fp32_spread":
                              bool(f32["median_ms"] - b16["median_ms"] > f32["max_ms"] - f32["min_ms"]),
                          "loss": float(loss[0].cpu())}), flush=True)
        return
    for _ in range(a.warmup):
        eng.train_step(img, target(False), micro_batch=mb)
        eng.adamw_step(1e-5, 1e-5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = eng.train_step(img, target(True), micro_batch=mb)
        eng.adamw_step(1e-5, 1e-5)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    if teacher is not None:  # the timed loop held the teacher too: the student's share is what is left
        it = dt * 1e3
        dt -= sum(t_ms) / len(t_ms) / 1e3
        head = {**head, "teacher": a.teacher, "teacher_ms": stats(t_ms), "iteration_ms": round(it, 2)}
    print(json.dumps({**head, "dtype": a.dtype, "attention": a.attention, "weight_grad": a.weight_grad,
                      "slice": eng.slice_size(a.batch) if mb is None else mb, "ms_per_step": round(dt * 1e3, 2),
                      "images_per_s": round(a.batch / dt, 3), "tflop_per_step": round(fl / 1e12, 2),
                      "tflops": round(fl / dt / 1e12, 2), "fraction_of_fp32_peak": round(fl / dt / PEAK_FP32, 3),
                      "loss": float(loss[0].cpu())}), flush=True)


if __name__ == "__main__":
    main()
