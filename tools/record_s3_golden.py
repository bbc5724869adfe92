"""Record the bits of one stage-3 step at the checkpoint's own position grid as sha256 digests:
tests/golden/s3_step_parent.json, which `test_equal_grid_bits_equal_the_parent` of tests/test_gpu_stage3_grid.py holds every
later build to -- through the entry points without a position grid and through the `_pos` ones called with g0 = the run's
grid.

    python tools/record_s3_golden.py [--tree PATH_OF_ANOTHER_CHECKOUT] [--out FILE] [--repeat N]

`--tree`: import dvt_amd from another checkout of the project (its library built), e.g. the parent commit of a change that
must not alter these bits.  Needs an MI355X; digests are specific to the GPU architecture and the compiler.

The step is `problem(384, 2, 98, 2)` of tests/test_gpu_stage3.py (restated below, same seeds) without registers and with 4:
a fresh engine, one `train_step` with the features written.  Every case runs `--repeat` times on fresh engines.

The loss and the LayerScale / LayerNorm parameter gradients (`is_atomic`) are reduced with float atomics (s2_loss_kernel,
s3_ls_bwd_kernel, s2_ln_bwd_kernel), whose order the hardware picks: the recorded build does not reproduce their bits
itself, so no later build can be held to them.  They are recorded under "varies" as the first repeat's values (base64 of
the fp32 bytes) and `spread`, the largest elementwise distance of any repeat from them -- the build's own run-to-run error;
`tolerance` is what the test allows.  Every other tensor must come out with the same bits in every repeat (the recorder
stops if one does not) and is recorded as its digest ("cases").
"""
import argparse
import base64
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CASES = {"reg0": 0, "reg4": 4}
DIM, DEPTH, IMG, BATCH = 384, 2, 98, 2


def digest(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def problem(torch, n_reg, seed=0):
    from dvt_amd.vit import random_state_dict
    g = (IMG - 14) // 14 + 1
    sd = random_state_dict(DIM, DEPTH, 14, (0 if n_reg else 1) + g * g, seed=seed, well_conditioned=True, n_reg=n_reg)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(BATCH, 3, IMG, IMG, generator=gen)
    t = torch.randn(BATCH, g, g, DIM, generator=gen)
    return sd, x, t


def step_tensors(torch, n_reg, **engine_kw) -> dict:
    """{"loss", "feat", "grads.<name>"...} (CPU) of one step of a fresh engine; `engine_kw` goes to Stage3Engine."""
    from dvt_amd import s3
    sd, x, t = problem(torch, n_reg)
    eng = s3.Stage3Engine(s3.make_config(DIM, DEPTH, 14, 14, IMG, IMG, n_reg), torch.device(DEV), **engine_kw)
    eng.load_timm(sd)
    feat = torch.empty(t.shape, device=DEV)
    loss = eng.train_step(x.to(DEV), t.to(DEV), feat)
    out = {"loss": loss.cpu().clone(), "feat": feat.cpu()}
    out.update({"grads." + k: v.cpu().clone() for k, v in eng.views(eng.grads).items()})
    return out


def is_atomic(name: str) -> bool:
    """Reduced over the token rows with float atomics: the loss terms, LayerNorm weight / bias, LayerScale gamma."""
    return name == "loss" or any(t in name for t in (".norm1.", ".norm2.", "grads.norm.", ".ls1.", ".ls2."))


def tolerance(values, spread: float) -> float:
    """Elementwise distance from the recorded values that the test allows: twice the recorded build's own run-to-run spread,
    and no less than twice 4 ulp of the tensor's largest value (a tensor whose repeats happened to agree still moves by a few
    ulp of its partial sums when the atomics land in another order)."""
    return 2.0 * max(spread, 4 * 2.0 ** -23 * float(values.abs().max()))


def unpack(torch, rec: dict):
    """A "varies" entry -> (values, spread)."""
    import numpy as np
    v = np.frombuffer(base64.b64decode(rec["values"]), dtype=np.float32).reshape(rec["shape"])
    return torch.from_numpy(v.copy()), float(rec["spread"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "s3_step_parent.json"))
    ap.add_argument("--repeat", type=int, default=16)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "denoising-vit_amd"))
    import torch
    cases, varies = {}, {}
    for name, n_reg in CASES.items():
        runs = [step_tensors(torch, n_reg) for _ in range(max(1, a.repeat))]
        moved = [k for k, v in runs[0].items() if not is_atomic(k) and not all(torch.equal(r[k], v) for r in runs)]
        if moved:
            raise SystemExit(f"{name}: {moved} are not reduced with atomics, yet their bits differ between repeats")
        cases[name] = {k: digest(v) for k, v in runs[0].items() if not is_atomic(k)}
        varies[name] = {k: {"shape": list(v.shape), "spread": max(float((r[k] - v).abs().max()) for r in runs),
                            "values": base64.b64encode(v.contiguous().numpy().tobytes()).decode()}
                        for k, v in runs[0].items() if is_atomic(k)}
    rec = {"what": "one train_step of a fresh Stage3Engine at the table's own grid: loss (4 floats), feat, and every gradient "
                   "tensor; problem(384, 2, 98, 2) of tests/test_gpu_stage3.py, n_reg 0 / 4, restated in "
                   "tools/record_s3_golden.py.  cases: sha256 of the fp32 bytes (every repeat gave the same); varies: the tensors "
                   "reduced with float atomics, first repeat's values and the largest distance of a repeat from them",
           "device": torch.cuda.get_device_name(0), "repeat": a.repeat, "cases": cases, "varies": varies}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"device": rec["device"], "stable": {k: len(v) for k, v in cases.items()},
                      "varies": {k: {n: r["spread"] for n, r in v.items()} for k, v in varies.items()}}))


if __name__ == "__main__":
    main()
