"""Child processes of the video-demo GPU tests: every GPU step that runs the extractor at the demo shape (490 x 854, stride 4:
25 321 tokens) runs in a process of its own under the parent's time limit, so that trouble ends it.

    python -m tests.video_gpu_child forward DIM DEPTH N_REG DTYPE OUT.npy
    python -m tests.video_gpu_child wrapper DTYPE
    python -m tests.video_gpu_child engine OUT.npz
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "denoising-vit_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

H, W, PATCH, STRIDE = 490, 854, 14, 4


def demo_case(dim: int, depth: int, n_reg: int):
    """(state dict, image) of a case: seeded on the host, so parent and child build the same ones."""
    from dvt_amd.vit import random_state_dict
    sd = random_state_dict(dim, depth, PATCH, (0 if n_reg else 1) + 37 * 37, seed=dim + depth, well_conditioned=True, n_reg=n_reg)
    img = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(7))
    return sd, img


GOLDEN = os.path.join(ROOT, "tests", "golden")
FRAMES = [os.path.join(GOLDEN, "davis-mallard-water", f) for f in ("00000.jpg", "00040.jpg")]


def engine_step(out: str) -> int:
    """The engine end to end on the two committed frames (random ViT-B/14, seed 0, bf16 extractor): frame 0 fitted twice,
    both frames applied; everything the parent compares goes into one .npz."""
    from dvt_amd import video as VD
    from dvt_amd import video_demo as D
    from dvt_amd.models import PretrainedViTWrapper
    dev = torch.device("cuda:0")
    vit = PretrainedViTWrapper("vit_base_patch14_dinov2.lvd142m", stride=STRIDE, img_size=(H, W), allow_random_init=True,
                               dtype="bfloat16")
    stats = VD.load_stats(os.path.join(GOLDEN, "video_stats.npz"))
    eng = VD.VideoDemoEngine(dev, (120, 211), 768, (H, W), stats, num_clusters=8, seed=0)
    imgs = [D.load_frame(f, H, W) for f in FRAMES]
    feats = [vit.features_nhwc(im[None].to(dev)).clone() for im in imgs]
    fit1 = {k: v.clone() for k, v in eng.fit(feats[0]).items()}
    eng.vis.work.view(torch.float32).fill_(float("nan"))
    fit2 = eng.fit(feats[0])
    same = all(torch.equal(fit1[k], fit2[k]) for k in fit1)
    keep = {"fit_twice_identical": np.asarray(same)}
    for k, v in fit2.items():
        keep[f"fit.{k}"] = v.cpu().numpy()
    for i, (im, f) in enumerate(zip(imgs, feats)):
        pics, det = eng.frame(f, image=im.to(dev), details=True)
        torch.cuda.synchronize()
        keep[f"{i}.feats"] = f.reshape(-1, 768).cpu().numpy()
        keep[f"{i}.image"] = im.numpy()
        for k, v in pics.items():
            keep[f"{i}.full.{k}"] = v.cpu().numpy()
        for k, v in det["token"].items():
            keep[f"{i}.token.{k}"] = v.cpu().numpy()
        for k in ("P", "norms", "labels", "mask_fg", "mask_standard", "range", "range_second", "norm_map"):
            keep[f"{i}.{k}"] = det[k].cpu().numpy()
    np.savez(out, **keep)
    print(f"engine: {eng.launches} launches in all, fit twice identical: {same}", flush=True)
    return 0


def main(argv) -> int:
    if argv[0] == "forward":
        from dvt_amd.vit import HipViT
        dim, depth, n_reg, dtype, out = int(argv[1]), int(argv[2]), int(argv[3]), argv[4], argv[5]
        sd, img = demo_case(dim, depth, n_reg)
        vit = HipViT(sd, PATCH, STRIDE, (H, W), "cuda:0", dtype=dtype)
        cfg = vit.cfg
        print(f"grid {cfg.grid_h} x {cfg.grid_w}, tokens {cfg.n_tokens}, s_pad {cfg.s_pad}, workspace "
              f"{vit.workspace_bytes(1) / 2**20:.0f} MiB", flush=True)
        got = vit.forward_features(img.to("cuda:0"))
        torch.cuda.synchronize()
        np.save(out, got.cpu().numpy())
        return 0
    if argv[0] == "wrapper":
        from dvt_amd.models import PretrainedViTWrapper
        vit = PretrainedViTWrapper("vit_base_patch14_dinov2.lvd142m", stride=STRIDE, img_size=(H, W), allow_random_init=True,
                                   dtype=argv[1])
        img = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(8)).to("cuda:0")
        out = vit.get_intermediate_layers(img, n=[vit.last_layer_index], reshape=True, norm=True)[-1].permute(0, 2, 3, 1)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (1, 120, 211, 768), tuple(out.shape)
        assert bool(torch.isfinite(out).all()), "non-finite tokens"
        print(f"wrapper {argv[1]}: {tuple(out.shape)} finite, |x| mean {float(out.norm(dim=-1).mean()):.3f}", flush=True)
        return 0
    if argv[0] == "engine":
        return engine_step(argv[1])
    raise SystemExit(f"unknown step {argv[0]!r}")


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
