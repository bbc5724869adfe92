"""Record the bits of one training step and one forward of the two linear-probe heads (dvt_amd.seg.SegHeadEngine,
dvt_amd.depth.DepthHeadEngine) as sha256 digests: tests/golden/heads_parent.json, which `test_step_bits_equal_the_parent`
of tests/test_gpu_seg_eval.py and tests/test_gpu_depth_eval.py hold every later build to.  Both heads reduce in a fixed
order, so their results are reproducible bit for bit.

    python tools/record_head_golden.py [--tree PATH_OF_ANOTHER_CHECKOUT] [--out FILE]

`--tree`: import dvt_amd from another checkout of the project (its library built), e.g. the parent commit of a change that
must not alter these bits.  Needs an MI355X; digests are specific to the GPU architecture and the compiler.

The heads and batches are the `make_head` / `make_batch` recipes of the two test files, restated with the seeds below.
Shapes: the smallest that reach every edge of the 64 x 64 logits tile and of the 256-row parameter-gradient slab --
  seg    C 384, K 21 / 150, B 3, 9 x 11 tokens (297 rows: five row tiles, slabs of 256 + 41), labels 45 x 61
  depth  C 384, B 3, 9 x 11 tokens, ground truth 45 x 61, it 0 / 100 (one ragged slab per image, the B >= 3 gradient loss)
  depth  C 768, B 2, 30 x 39 tokens, ground truth 416 x 544 (five slabs per image, 4 x 256 + 146)
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SEG_CASES = [(384, 21), (384, 150)]                                            # (C, K); B 3, 9 x 11 tokens, labels 45 x 61
DEPTH_CASES = [(384, 3, 9, 11, 45, 61, 0), (384, 3, 9, 11, 45, 61, 100), (768, 2, 30, 39, 416, 544, 100)]  # C B h w H W it


def digest(*tensors) -> str:
    return hashlib.sha256(b"".join(t.detach().cpu().contiguous().numpy().tobytes() for t in tensors)).hexdigest()


def seg_head(torch, C, K, seed):
    from dvt_amd.seg import SegHeadEngine
    eng = SegHeadEngine(C, K, DEV, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    v = eng.views()
    v["conv_seg.weight"].mul_(20.0)
    v["conv_seg.bias"].copy_(torch.randn(K, generator=g) * 0.1)
    v["bn.weight"].copy_(1.0 + 0.2 * torch.randn(C, generator=g))
    v["bn.bias"].copy_(0.2 * torch.randn(C, generator=g))
    eng.running.copy_(torch.cat([torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)]))
    return eng


def seg_batch(torch, B, h, w, C, K, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, h, w, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
    lab = torch.randint(0, K, (B, H, W), generator=g, dtype=torch.int64).to(torch.uint8)
    lab[:, :3] = 255
    lab[:, :, W - 5:] = 255
    return x.to(DEV).contiguous(), lab.to(DEV).contiguous()


def depth_head(torch, C, seed):
    from dvt_amd.depth import DepthHeadEngine
    eng = DepthHeadEngine(C, DEV, seed=seed)
    eng.views()["conv_depth.weight"].mul_(3.0)
    return eng


def depth_batch(torch, B, h, w, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, h, w, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + 0.3 * torch.randn(C, generator=g)
    cls = torch.randn(B, C, generator=g)
    gt = 0.5 + 8.0 * torch.rand(B, H, W, generator=g)
    gt[torch.rand(B, H, W, generator=g) < 0.1] = 0.0
    gt[:, :3] = 0.0
    gt[:, :, W - 4:] = 0.0
    return x.to(DEV).contiguous(), cls.to(DEV).contiguous(), gt.to(DEV).contiguous()


def seg_digests(eng, x, lab) -> dict:
    out = eng.train_step(x, lab)
    return {"step": digest(out, eng.grads, eng.running), "forward": digest(eng.forward(x))}


def depth_digests(eng, x, cls, gt, it) -> dict:
    out = eng.train_step(x, cls, gt, it)
    return {"step": digest(out, eng.grads), "forward": digest(eng.forward(x, cls))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "heads_parent.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "denoising-vit_amd"))
    import torch
    seg, depth = {}, {}
    for C, K in SEG_CASES:
        x, lab = seg_batch(torch, 3, 9, 11, C, K, 45, 61, seed=3)
        seg[f"C{C}_K{K}"] = seg_digests(seg_head(torch, C, K, seed=C + K), x, lab)
    for C, B, h, w, H, W, it in DEPTH_CASES:
        x, cls, gt = depth_batch(torch, B, h, w, C, H, W, seed=B + it)
        depth[f"C{C}_B{B}_{h}x{w}_it{it}"] = depth_digests(depth_head(torch, C, seed=C + B), x, cls, gt, it)
    rec = {"what": "sha256 of the fp32 bytes: step = (out, grads[, running]) after one train_step of a fresh head, forward = "
                   "forward(x[, cls]) after it; heads and batches: make_head / make_batch of tests/test_gpu_seg_eval.py and "
                   "tests/test_gpu_depth_eval.py, seeds as in tools/record_head_golden.py",
           "device": torch.cuda.get_device_name(0), "seg": seg, "depth": depth}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
