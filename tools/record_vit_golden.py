"""Record the bits of a 2-block ViT-B/14 forward (518 x 518, 2 views, bf16 and fp32 extractors, with and without registers)
as sha256 digests: tests/golden/vitb_2block_parent.json, which tests/test_gpu_vitg.py holds every later build to.

    python tools/record_vit_golden.py [--tree PATH_OF_ANOTHER_CHECKOUT] [--out FILE]

`--tree`: import dvt_amd from another checkout of the project (its library built), e.g. the parent commit of a change that
must not alter these bits.  Needs an MI355X; digests are specific to the GPU architecture and the compiler.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "vitb_2block_parent.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "denoising-vit_amd"))
    import torch
    from dvt_amd.vit import HipViT, random_state_dict
    dev = "cuda"
    out = {}
    for n_reg in (0, 4):
        sd = random_state_dict(768, 2, 14, (0 if n_reg else 1) + 37 * 37, seed=9, well_conditioned=True, n_reg=n_reg)
        x = torch.randn(2, 3, 518, 518, generator=torch.Generator().manual_seed(12)).to(dev)
        for dtype in ("bfloat16", "float32"):
            feat, cls = HipViT(sd, 14, 14, (518, 518), dev, dtype=dtype).forward_features(x, return_cls=True)
            out[f"{dtype}_reg{n_reg}"] = hashlib.sha256(feat.cpu().numpy().tobytes() + cls.cpu().numpy().tobytes()).hexdigest()
    rec = {"what": "sha256(feat bytes + cls bytes) of HipViT.forward_features(return_cls=True): ViT-B/14, 2 blocks, "
                   "random_state_dict(768, 2, 14, n_tokens, seed=9, well_conditioned=True, n_reg), x = randn(2, 3, 518, 518) seed 12",
           "device": torch.cuda.get_device_name(0), "sha256": out}
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
