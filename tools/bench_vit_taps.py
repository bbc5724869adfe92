"""Four layers of ViT-B/14 from ONE tapped forward against the four forwards get_intermediate_layers ran before.

ViT-B/14 (random weights) at 518 x 518, 32 views, layers [2, 5, 8, 11] -- the out_indices of the reference's dense-task heads
(evaluation/eval_utils/misc.py:140-182).  By block count the old path runs 3 + 6 + 9 + 12 = 30 blocks, four patch embeddings
and four final norms, the tapped one 12 blocks, one patch embedding and four tap launches.  Both legs
write the same bits (checked before timing).  bf16 and exact fp32; the legs are interleaved in one process, every sample is one
call between two device events, the median of `--reps` samples is reported.  Prints one JSON line and writes it to `--out`.

    python tools/bench_vit_taps.py [--views 32] [--reps 10] [--out profiles/taps/bench_vit_taps.json]

Run it under a time limit of its own (`timeout -k 10 400 python tools/bench_vit_taps.py`).
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

LAYERS = [2, 5, 8, 11]


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "taps", "bench_vit_taps.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"model": "vit_base_patch14_dinov2.lvd142m", "weights": "random", "image": 518, "views": a.views, "layers": LAYERS,
           "reps": a.reps, "blocks_four_forwards": sum(i + 1 for i in LAYERS), "blocks_tapped": LAYERS[-1] + 1}
    x = torch.randn(a.views, 3, 518, 518, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    for dtype in ("bfloat16", "float32"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            w = PretrainedViTWrapper("vit_base_patch14_dinov2.lvd142m", stride=14, allow_random_init=True, dtype=dtype)
        eng = w._engine(dev)
        old_maps = [torch.empty(a.views, 37, 37, 768, device=dev) for _ in LAYERS]
        new_maps = [torch.empty(a.views, 37, 37, 768, device=dev) for _ in LAYERS]

        def four_forwards():
            for i, m in zip(LAYERS, old_maps):
                eng.forward_features(x, n_blocks=i + 1, out=m)

        def tapped():
            eng.forward_taps(x, LAYERS, outs=new_maps)

        legs = {"four_forwards": four_forwards, "tapped": tapped}
        for fn in legs.values():  # warm-up; and the two legs write the same bits
            fn()
        torch.cuda.synchronize()
        same = all(torch.equal(o, n) for o, n in zip(old_maps, new_maps))
        times = {k: [] for k in legs}
        for _ in range(a.reps):  # interleaved: every repetition times every leg once
            for k, fn in legs.items():
                times[k].append(timed(fn))
        res = {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in times.items()}
        res["same_bits"] = same
        res["tapped_over_four_forwards"] = res["tapped"]["ms_median"] / res["four_forwards"]["ms_median"]
        res["launch_plan"] = eng.launch_plan(a.views)
        out[dtype] = res
        del w, eng, old_maps, new_maps
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
