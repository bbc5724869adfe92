"""Record the bits of the stage-2 denoiser's step and forward as sha256 digests: tests/golden/s2_parent_digests.json, which
`test_step_keeps_the_parents_bits` of tests/test_gpu_stage2.py holds every later build to.

    python tools/record_s2_parent_digests.py [--tree PATH_OF_ANOTHER_CHECKOUT] [--out FILE] [--repeat N]

`--tree`: import dvt_amd from another checkout of the project (its library built): the parent commit of a change that must
not alter these bits.  Needs an MI355X; digests are specific to the GPU architecture and the compiler.

Cases (CASES below): the smallest shapes that reach every branch of the block code the stage-2 and stage-3 steps share
(csrc/dvt_block_train.hip).  Models and batches are `make_pair` of tests/test_gpu_stage2.py with the seeds of its
`test_step_gradients_vs_autograd` (restated below).  A step case records the loss and every gradient tensor of one
`training_step` of a fresh model; the forward case records `pred` of one inference forward.

What is a digest and what is a value with a tolerance follows tools/record_s3_golden.py, whose `digest`, `is_atomic`,
`unpack` and `tolerance` this script uses.  A tensor is recorded under "varies" (first repeat's values and the recording
build's run-to-run spread) when `is_atomic` names it -- the loss and the LayerNorm parameter gradients, summed with float
atomics -- or when its bits moved between the `--repeat` runs (the k-split weight gradients that accumulate with atomics on
the 64 x 64 tile); "observed" lists the latter per case.  Every other tensor came out with the same bits in every repeat and
is recorded as its digest.  The recorder stops if one of MUST_BE_STABLE moves in the default case.
"""
import argparse
import base64
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
# name: (h, w, dim, blocks, batch, dvt_tune_set(18, mask), what is recorded)
CASES = {
    "rows11x11": (11, 11, 384, 2, 3, 63, "step"),   # Tp 128: attention-row kernel both ways, 128-row tiles, forks
    "gemm7x7": (7, 7, 384, 1, 3, 63, "step"),       # Tp 64: GEMM + softmax forward, softmax backward as the GEMM epilogue
    "mask0_11x11": (11, 11, 384, 2, 3, 0, "step"),  # 64 x 64 tiles, unfused softmax backward, no fork
    "forward5x9": (5, 9, 384, 2, 2, 63, "forward"),  # inference: block inputs ping-pong
}
MUST_BE_STABLE = ("rows11x11", [f"grads.denoiser.0.{n}.weight" for n in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")]
                  + ["grads.pos_embed"])


def helpers():
    spec = importlib.util.spec_from_file_location("record_s3_golden", os.path.join(ROOT, "tools", "record_s3_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_pair(torch, h, w, c, blocks, seed):
    """`make_pair` of tests/test_gpu_stage2.py: the oracle's initial state with perturbed LayerNorm parameters."""
    if ROOT not in sys.path:
        sys.path.append(ROOT)
    from oracle import stage2 as O
    from dvt_amd.models import Denoiser
    torch.manual_seed(seed)
    ref = O.Denoiser(h, w, c, True, blocks)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    mine = Denoiser(h, w, c, None, True, blocks, device=torch.device(DEV))
    mine.load_state_dict(ref.state_dict())
    return mine


def step_tensors(torch, case: str) -> dict:
    """{"loss", "grads.<name>"...} of one training_step of a fresh model, or {"pred"} of one forward (CPU tensors)."""
    from dvt_amd import _lib
    h, w, c, blocks, batch, mask, what = CASES[case]
    mine = make_pair(torch, h, w, c, blocks, seed=1)
    torch.manual_seed(2)
    x, t = torch.randn(batch, h, w, c), torch.randn(batch, h, w, c)
    _lib.check(_lib.lib().dvt_tune_set(18, mask), "dvt_tune_set")
    try:
        if what == "forward":
            return {"pred": mine(x.to(DEV)).cpu().clone()}
        out = {"loss": mine.training_step(x.to(DEV), t.to(DEV)).cpu().clone()}
        out.update({"grads." + k: v.cpu().clone() for k, v in mine.engine.views(mine.engine.grads).items()})
        return out
    finally:
        _lib.check(_lib.lib().dvt_tune_set(18, 63), "dvt_tune_set")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "s2_parent_digests.json"))
    ap.add_argument("--repeat", type=int, default=8)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "denoising-vit_amd"))
    import torch
    H = helpers()
    cases, varies, observed = {}, {}, {}
    for name in CASES:
        runs = [step_tensors(torch, name) for _ in range(max(1, a.repeat))]
        moved = [k for k, v in runs[0].items() if not H.is_atomic(k) and not all(torch.equal(r[k], v) for r in runs)]
        if name == MUST_BE_STABLE[0] and set(moved) & set(MUST_BE_STABLE[1]):
            raise SystemExit(f"{name}: {sorted(set(moved) & set(MUST_BE_STABLE[1]))} differ between repeats")
        loose = [k for k in runs[0] if H.is_atomic(k) or k in moved]
        observed[name] = moved
        cases[name] = {k: H.digest(v) for k, v in runs[0].items() if k not in loose}
        varies[name] = {k: {"shape": list(runs[0][k].shape), "spread": max(float((r[k] - runs[0][k]).abs().max()) for r in runs),
                            "values": base64.b64encode(runs[0][k].contiguous().numpy().tobytes()).decode()} for k in loose}
    rec = {"what": "one training_step (loss, 4 floats, and every gradient tensor) or one forward (pred) of a fresh stage-2 "
                   "Denoiser per case of tools/record_s2_parent_digests.py.  cases: sha256 of the fp32 bytes (every repeat "
                   "gave the same); varies: first repeat's values and the largest distance of a repeat from them, for the "
                   "tensors reduced with float atomics by construction (loss, LayerNorm parameters) and for those listed "
                   "under observed, whose bits moved between the repeats",
           "device": torch.cuda.get_device_name(0), "repeat": a.repeat, "cases": cases, "varies": varies, "observed": observed}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"device": rec["device"], "stable": {k: len(v) for k, v in cases.items()}, "observed": observed,
                      "varies": {k: {n: r["spread"] for n, r in v.items()} for k, v in varies.items()}}))


if __name__ == "__main__":
    main()
