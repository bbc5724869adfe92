"""Record the bits of one default (exact-fp32) stage-3 step through `dvt_s3_train_step` as sha256 digests:
tests/golden/s3_parent_digests.json, which `test_default_path_keeps_the_parents_bits` of tests/test_gpu_stage3_bf16.py holds
every later build to -- through `dvt_s3_train_step` and through `dvt_s3_train_slice_pos_mp` with gemm_mode 0.

    python tools/record_s3_parent_digests.py [--tree PATH_OF_ANOTHER_CHECKOUT] [--out FILE] [--repeat N] [--bf16 [--attention]]

`--tree`: import dvt_amd from another checkout of the project (its library built): the parent commit of a change that must
not alter these bits.  Needs an MI355X; digests are specific to the GPU architecture and the compiler.

Cases: `problem(dim, depth, 98, 2)` of tests/test_gpu_stage3.py (same seeds) at (384, 2) and (768, 1), no registers.
What is a digest and what is a value with a tolerance follows tools/record_s3_golden.py, whose helpers this script uses:
the loss and the LayerNorm / LayerScale parameter gradients are summed with float atomics and do not reproduce their own
bits from run to run, so they are recorded as values with the recording build's spread over `--repeat` runs; every other
gradient tensor must come out with the same bits in every repeat and is recorded as its digest.

`--bf16`: the opt-in bf16 mode instead (route "mp1": gemm_mode 1 through `Stage3Engine(dtype="bfloat16")`) at its smallest case,
s384x2, into tests/golden/s3_bf16_parent_digests.json, which `test_bf16_path_keeps_the_parents_bits` holds.  Same rule, except
that a tensor `is_atomic` does not name whose bits moved between the repeats is recorded under "varies" too and listed under
"observed", as tools/record_s2_parent_digests.py does, instead of stopping the recorder.

`--bf16 --attention`: the same for the bf16 flash attention on top (route "mp3": gemm_mode 3 through
`Stage3Engine(dtype="bfloat16", attention="bfloat16")`) into tests/golden/s3_bf16_attn_parent_digests.json, which
`test_bf16_attention_path_keeps_the_parents_bits` of tests/test_gpu_stage3_wgrad.py holds.
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CASES = {"s384x2": (384, 2), "b768x1": (768, 1)}
IMG, BATCH = 98, 2


def helpers():
    spec = importlib.util.spec_from_file_location("record_s3_golden", os.path.join(ROOT, "tools", "record_s3_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def problem(torch, dim, depth, seed=0):
    from dvt_amd.vit import random_state_dict
    g = (IMG - 14) // 14 + 1
    sd = random_state_dict(dim, depth, 14, 1 + g * g, seed=seed, well_conditioned=True)
    gen = torch.Generator().manual_seed(seed + 1)
    return sd, torch.randn(BATCH, 3, IMG, IMG, generator=gen), torch.randn(BATCH, g, g, dim, generator=gen)


def step_tensors(torch, case: str, route: str = "step") -> dict:
    """{"loss", "grads.<name>"...} (CPU) of one step of a fresh fp32 engine.  route "step": `dvt_s3_train_step` (what
    Stage3Engine.train_step calls for a whole batch); "mp0": `dvt_s3_train_slice_pos_mp` with g0 = 0 and gemm_mode 0; "mp1":
    the bf16 engine's train_step, the same entry point with gemm_mode 1; "mp3": with the bf16 attention too, gemm_mode 3."""
    from dvt_amd import _lib, s3
    dim, depth = CASES[case]
    sd, x, t = problem(torch, dim, depth)
    eng = s3.Stage3Engine(s3.make_config(dim, depth, 14, 14, IMG, IMG), torch.device(DEV),
                          **({"mp1": dict(dtype="bfloat16"), "mp3": dict(dtype="bfloat16", attention="bfloat16")}.get(route, {})))
    eng.load_timm(sd)
    x, t = x.to(DEV), t.to(DEV)
    if route != "mp0":
        loss = eng.train_step(x, t)
    else:
        w = eng._workspace(eng.workspace_bytes(BATCH))
        loss = eng.loss
        _lib.check(_lib.lib().dvt_s3_train_slice_pos_mp(C.byref(eng.cfg), 0, None, None, 0, _lib.ptr(eng.params),
                                                        _lib.ptr(eng.grads), _lib.ptr(x), _lib.ptr(t), None, BATCH, BATCH,
                                                        _lib.ptr(w), w.numel(), _lib.ptr(loss), _lib.stream()),
                   "dvt_s3_train_slice_pos_mp")
    out = {"loss": loss.cpu().clone()}
    out.update({"grads." + k: v.cpu().clone() for k, v in eng.views(eng.grads).items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--attention", action="store_true", help="with --bf16: the bf16 flash attention too (gemm_mode 3)")
    a = ap.parse_args()
    if a.attention and not a.bf16:
        raise SystemExit("--attention records gemm_mode 3, which is built on --bf16")
    a.out = a.out or os.path.join(ROOT, "tests", "golden", ("s3_bf16_attn_parent_digests.json" if a.attention else
                                                            "s3_bf16_parent_digests.json") if a.bf16 else "s3_parent_digests.json")
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "denoising-vit_amd"))
    import base64

    import torch
    H = helpers()
    cases, varies, observed = {}, {}, {}
    for name in (["s384x2"] if a.bf16 else CASES):
        runs = [step_tensors(torch, name, ("mp3" if a.attention else "mp1") if a.bf16 else "step") for _ in range(max(1, a.repeat))]
        moved = [k for k, v in runs[0].items() if not H.is_atomic(k) and not all(torch.equal(r[k], v) for r in runs)]
        if moved and not a.bf16:
            raise SystemExit(f"{name}: {moved} are not reduced with atomics, yet their bits differ between repeats")
        observed[name] = moved
        cases[name] = {k: H.digest(v) for k, v in runs[0].items() if not H.is_atomic(k) and k not in moved}
        varies[name] = {k: {"shape": list(v.shape), "spread": max(float((r[k] - v).abs().max()) for r in runs),
                            "values": base64.b64encode(v.contiguous().numpy().tobytes()).decode()}
                        for k, v in runs[0].items() if H.is_atomic(k) or k in moved}
    rec = {"what": (f"one train_step of a fresh bf16 Stage3Engine (gemm_mode {3 if a.attention else 1})" if a.bf16 else
                    "one dvt_s3_train_step of a fresh fp32 Stage3Engine") + ": loss (4 floats) and every gradient tensor; "
                   "problem(dim, depth, 98, 2) of tests/test_gpu_stage3.py at (384, 2) and (768, 1), restated in "
                   "tools/record_s3_parent_digests.py.  cases: sha256 of the fp32 bytes (every repeat gave the same); varies: "
                   "the tensors reduced with float atomics, first repeat's values and the largest distance of a repeat from them",
           "device": torch.cuda.get_device_name(0), "repeat": a.repeat, "cases": cases, "varies": varies}
    if a.bf16:
        rec["observed"] = observed  # not atomics by construction, yet their bits moved between the repeats: under varies
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"device": rec["device"], "stable": {k: len(v) for k, v in cases.items()},
                      "varies": {k: {n: r["spread"] for n, r in v.items()} for k, v in varies.items()}}))


if __name__ == "__main__":
    main()
