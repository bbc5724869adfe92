"""Stage-2 (N3) step benchmark: BASELINE configs[4] shapes -- ViT-B/14 feature maps 37 x 37 x 768, one Block,
batch 32 per GPU (main_denoiser.py:43) -- forward + loss + backward + (all-reduce) + AdamW per step on synthetic
pairs resident in HBM.  One process per GPU (`python -m torch.distributed.run --nproc-per-node N tools/bench_stage2.py`).
Prints one JSON line; not the repository's headline metric (bench.py measures stage 1).

`--ab N`: an interleaved A/B of the step's arithmetics in one process on one engine (single GPU) -- exact fp32, gemm_mode 1
(bf16 GEMMs), 3 (+ bf16 flash attention) and 7 (+ bf16 split-K weight gradients), one step of each in turn, N timed steps of
each after the warm-up of all, every step timed on its own with the device synchronised on both sides (the chip's clock
drifts over a run: alternating steps see the same clock).  The JSON line carries per leg the median, minimum and maximum ms
per step and the workspace bytes per sample (the increment from batch 1 to batch 2), and per bf16 leg whether its median lies
below the fp32 median by more than the fp32 leg's own min..max spread.  All legs run on rows padded to 128, which at
37 x 37 is the default padding too (1408 rows).
`--feeder N`: additionally time `dvt_amd.stage2.BatchFeeder` alone over synthetic .npy pairs of the benchmark's shape written
to a temporary directory, N batches after one of warm-up, in samples/s: what the host can feed a step."""
import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "denoising-vit_amd")]
from dvt_amd import dist as D  # noqa: E402
from dvt_amd.models import Denoiser  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--blocks", type=int, default=1)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--grid", type=int, default=37)
ap.add_argument("--stages", type=int, default=0, help="LDS stages of the GEMMs (2 / 3; 0 = library default)")
ap.add_argument("--ab", type=int, default=0, metavar="N", help="interleaved fp32 / mode 1 / 3 / 7 A/B, N timed steps of each")
ap.add_argument("--feeder", type=int, default=0, metavar="N", help="time the BatchFeeder alone over N batches of synthetic files")
ap.add_argument("--feeder_workers", type=int, default=8)
a = ap.parse_args()
rank, world, local = D.env_ranks()
dev = torch.device("cuda", local)
torch.cuda.set_device(dev)
D.init(dev, world)
if a.stages:
    from dvt_amd import _lib
    _lib.lib().dvt_tune_set(4, a.stages)
m = Denoiser(a.grid, a.grid, a.dim, None, True, a.blocks, device=dev, seed=0, train_dtype="bfloat16" if a.ab else "float32")
if world > 1:
    dist.broadcast(m.engine.params, src=0)
g = torch.Generator(device=dev).manual_seed(rank)
x = torch.randn(a.batch, a.grid, a.grid, a.dim, device=dev, generator=g)
t = torch.randn(a.batch, a.grid, a.grid, a.dim, device=dev, generator=g)


def step():
    loss = m.training_step(x, t)
    if world > 1:
        dist.all_reduce(m.engine.grads)
    m.engine.adamw_step(1e-4, 1e-5, grad_scale=1.0 / world)
    return loss


def feeder_rate():
    """samples/s of stage2.BatchFeeder alone: a.feeder batches of a.batch pairs from .npy files (as many pairs as two batches,
    cycled), the device copy included, nothing computed."""
    import shutil
    import tempfile
    import numpy as np
    from dvt_amd import stage2
    root = tempfile.mkdtemp(prefix="s2_feeder_")
    try:
        n = 2 * a.batch
        os.makedirs(f"{root}/denoised_features")
        os.makedirs(f"{root}/raw_features")
        rng = np.random.default_rng(0)
        for i in range(n):
            np.save(f"{root}/raw_features/{i}.npy", rng.standard_normal((1, a.grid, a.grid, a.dim), dtype=np.float32))
            np.save(f"{root}/denoised_features/{i}.npy", rng.standard_normal((a.grid, a.grid, a.dim), dtype=np.float32))
        with open(f"{root}/list.txt", "w") as f:
            f.write("".join(f"{i}.jpg 0\n" for i in range(n)))
        ds = stage2.PairedFeatureList(f"{root}/list.txt", f"{root}/denoised_features")
        fd = stage2.BatchFeeder(ds, stage2.sampler_indices(n, 1, 0, False), a.batch, (a.grid, a.grid, a.dim), dev,
                                workers=a.feeder_workers)
        try:
            fd.release(fd.next()[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.feeder):
                fd.release(fd.next()[0])
            torch.cuda.synchronize()
            return a.feeder * a.batch / (time.perf_counter() - t0)
        finally:
            fd.close()
    finally:
        shutil.rmtree(root, ignore_errors=True)


if a.ab > 0:
    if world > 1:
        raise SystemExit("--ab is a single-GPU measurement")
    eng = m.engine
    modes = {"float32": ("float32", "float32", "float32"), "mode1": ("bfloat16", "float32", "float32"),
             "mode3": ("bfloat16", "bfloat16", "float32"), "mode7": ("bfloat16", "bfloat16", "bfloat16")}
    per_sample = {}
    for name, mode in modes.items():
        eng.set_dtype(*mode)
        per_sample[name] = eng.workspace_bytes(2) - eng.workspace_bytes(1)
    ms = {name: [] for name in modes}
    for i in range(a.warmup + a.ab):
        for name, mode in modes.items():
            eng.set_dtype(*mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = step()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    legs = {}
    for name, v in ms.items():
        v = sorted(v)
        med = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
        legs[name] = {"median_ms": round(med, 3), "min_ms": round(v[0], 3), "max_ms": round(v[-1], 3),
                      "samples_per_s": round(a.batch / med * 1e3, 1), "workspace_bytes_per_sample": per_sample[name]}
    f32 = legs["float32"]
    spread = f32["max_ms"] - f32["min_ms"]
    out = {"bench": "stage2_step", "mode": "interleaved_ab", "steps_each": a.ab, "grid": a.grid, "dim": a.dim, "blocks": a.blocks,
           "batch": a.batch, "tokens_pad": eng.cfg.tokens_pad, **legs, "fp32_spread_ms": round(spread, 3),
           "loss": float(loss[0].cpu())}
    for name in ("mode1", "mode3", "mode7"):
        out[f"{name}_speedup"] = round(f32["median_ms"] / legs[name]["median_ms"], 3)
        out[f"{name}_faster_than_fp32_spread"] = bool(f32["median_ms"] - legs[name]["median_ms"] > spread)
    if a.feeder > 0:
        del m, eng
        torch.cuda.empty_cache()
        out["feeder_samples_per_s"] = round(feeder_rate(), 1)
        out["feeder_workers"] = a.feeder_workers
    print(json.dumps(out), flush=True)
    D.finish()
    sys.exit(0)

for _ in range(a.warmup):
    step()


def region():
    for _ in range(a.steps):
        step()
    return a.steps * a.batch


n, elapsed, per_rank = D.timed(region, dev)
C, T, F, H = a.dim, a.grid * a.grid, 4 * a.dim, a.dim // 64
lin = 2.0 * a.batch * T * (3 * C * C + C * C + 2 * C * F)   # forward linear layers
att = 4.0 * a.batch * H * T * T * 64                        # q k^T and P v
flops = 3.0 * (lin * a.blocks) + (att + 1.5 * att * 2) * a.blocks  # backward: 2x linear, 4 attention products
if rank == 0:
    print(json.dumps({
        "metric": "stage-2 denoiser training samples/s", "value": world * n / elapsed, "unit": "samples/s",
        "n_gpus": world, "steps": a.steps, "ms_per_step": 1e3 * elapsed / a.steps, "dtype": "f32",
        "config": {"workload": f"Denoiser({a.grid}x{a.grid}x{a.dim}, {a.blocks} block) fwd+loss+bwd+AdamW",
                   "batch_per_gpu": a.batch, "parallelism": f"dp{world}"},
        "algorithmic_tflop_per_step": flops / 1e12,
        "achieved_tflops_per_gpu": flops / (elapsed / a.steps) / 1e12,
        "loss": float(step()[0])}))
D.finish()
