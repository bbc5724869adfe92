"""GPU: `python -m dvt_amd.evaluate` end to end on a small synthetic VOC-format tree (training, checkpoints, slide
evaluation, eval_results.json), resume reproducibility, the --load-denoiser-from path, the SyncBN step on a merged
statistics record, and the ViT backbone's centre padding at a crop size other than 512."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
MIOU_MIN = 0.8  # measured 0.982 (200 iterations, random ViT-S); predicting background everywhere gives about 0.23


def write_voc(root, n_train=8, n_val=4, seed=0):
    """JPEG images of a grey background with a red and a green rectangle (classes 1 and 2), a 255 border in the labels."""
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "JPEGImages"))
    os.makedirs(os.path.join(root, "SegmentationClass"))
    os.makedirs(os.path.join(root, "ImageSets", "Segmentation"))
    names = {"train": [], "val": []}
    for split, n in (("train", n_train), ("val", n_val)):
        for i in range(n):
            name = f"{split}_{i:03d}"
            H, W = 96 + 8 * rng.randint(4), 128 + 8 * rng.randint(4)
            img = np.full((H, W, 3), 128, np.uint8) + rng.randint(-10, 10, (H, W, 3)).astype(np.uint8)
            lab = np.zeros((H, W), np.uint8)
            for cls, col in ((1, (220, 30, 30)), (2, (30, 200, 40))):
                h, w = rng.randint(H // 4, H // 2), rng.randint(W // 4, W // 2)
                y, x = rng.randint(0, H - h), rng.randint(0, W - w)
                img[y:y + h, x:x + w] = col
                lab[y:y + h, x:x + w] = cls
            lab[:3] = 255
            lab[:, -3:] = 255
            Image.fromarray(img).save(os.path.join(root, "JPEGImages", name + ".jpg"), quality=95)
            Image.fromarray(lab).save(os.path.join(root, "SegmentationClass", name + ".png"))
            names[split].append(name)
        with open(os.path.join(root, "ImageSets", "Segmentation", f"{split}.txt"), "w") as f:
            f.write("\n".join(names[split]) + "\n")


def run_eval(args, timeout=420):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "denoising-vit_amd"), ROOT, env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-m", "dvt_amd.evaluate", "voc2012_linear", "--allow_random_vit",
                        "--launcher", "none", "--seed", "0", *args], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


SHORT = ["lr_config.warmup_iters=20", "optimizer.lr=0.01", "log_config.interval=50"]


@pytest.fixture(scope="module")
def voc(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("voc"))
    write_voc(root)
    return root


@pytest.fixture(scope="module")
def full_run(voc, tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("full"))
    out = run_eval(["--data-root", voc, "--work-dir", wd, "--cfg-options", "runner.max_iters=200",
                    "checkpoint_config.interval=100", "evaluation.interval=200", *SHORT])
    return wd, out


def test_end_to_end_miou(full_run):
    wd, out = full_run
    res = json.load(open(os.path.join(wd, "eval_results.json")))
    assert len(res) == 1 and res[0]["iter"] == 200
    for k in ("aAcc", "mIoU", "mAcc", "IoU.background", "Acc.aeroplane"):
        assert k in res[0]
    print(f"synthetic VOC mIoU {res[0]['mIoU']:.4f} aAcc {res[0]['aAcc']:.4f}")
    assert res[0]["mIoU"] > MIOU_MIN, res[0]
    ck = torch.load(os.path.join(wd, "latest.pth"), weights_only=False)
    assert set(ck) == {"meta", "state_dict", "optimizer"} and ck["meta"]["iter"] == 200
    assert ck["state_dict"]["decode_head.conv_seg.weight"].shape == (21, 384, 1, 1)
    assert int(ck["state_dict"]["decode_head.bn.num_batches_tracked"]) == 200
    assert any(f.endswith(".log") and "per class results" in open(os.path.join(wd, f)).read() for f in os.listdir(wd))


def test_resume_reproduces_the_uninterrupted_run(voc, full_run, tmp_path):
    wd, _ = full_run
    run_eval(["--data-root", voc, "--work-dir", str(tmp_path), "--resume-from", os.path.join(wd, "iter_100.pth"),
              "--no-validate", "--cfg-options", "runner.max_iters=200", "checkpoint_config.interval=100", *SHORT])
    a = torch.load(os.path.join(wd, "iter_200.pth"), weights_only=False)
    b = torch.load(os.path.join(str(tmp_path), "iter_200.pth"), weights_only=False)
    for k, t in a["state_dict"].items():
        assert torch.equal(t, b["state_dict"][k]), k


def test_load_denoiser_from(voc, tmp_path):
    from dvt_amd.models.online_denoiser import Denoiser
    den = Denoiser(noise_map_height=37, noise_map_width=37, feat_dim=384, vit=None, num_blocks=1, device=DEV, seed=0)
    ck = str(tmp_path / "stage2.pth")
    torch.save({"denoiser": den.state_dict(), "step": 1}, ck)
    run_eval(["--data-root", voc, "--work-dir", str(tmp_path / "wd"), "--load-denoiser-from", ck,
              "--cfg-options", "runner.max_iters=10", "checkpoint_config.interval=10", "evaluation.interval=10", *SHORT])
    res = json.load(open(str(tmp_path / "wd" / "eval_results.json")))
    assert np.isfinite(res[0]["aAcc"])


def test_syncbn_step_on_merged_record_equals_whole_batch(built_lib):
    """Two 'ranks' each hold half the batch; stepping each half on the merged record, then averaging the gradients,
    is the whole batch's step (running statistics included)."""
    from dvt_amd.seg import SegHeadEngine
    C, K = 384, 21
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(4, 9, 11, C, generator=g) + 3 * torch.randn(C, generator=g)).to(DEV)
    lab = torch.randint(0, K, (4, 45, 61), generator=g).to(torch.uint8).to(DEV)
    whole = SegHeadEngine(C, K, DEV, seed=1)
    whole.views()["conv_seg.weight"].mul_(20)
    out_w = whole.train_step(x, lab).clone()
    ranks = [SegHeadEngine(C, K, DEV, seed=1) for _ in range(2)]
    for r in ranks:
        r.views()["conv_seg.weight"].mul_(20)
    halves = [(x[2 * i:2 * i + 2].contiguous(), lab[2 * i:2 * i + 2].contiguous()) for i in range(2)]
    merged = ranks[0].merge_stats(torch.stack([r.batch_stats(h[0]) for r, h in zip(ranks, halves)]))
    outs = [r.train_step(h[0], h[1], stats=merged).clone() for r, h in zip(ranks, halves)]
    grad = (ranks[0].grads + ranks[1].grads) / 2
    assert ((grad - whole.grads).norm() / whole.grads.norm()).item() < 1e-5
    assert abs(((outs[0][0] + outs[1][0]) / 2 - out_w[0]).item()) < 1e-5 * abs(out_w[0].item())
    for r in ranks:
        assert ((r.running - whole.running).norm() / whole.running.norm()).item() < 1e-6


def test_vit_backbone_centre_pads_other_crop_sizes(built_lib):
    from dvt_amd.seg import ViTBackbone
    from dvt_amd.vit import HipViT, random_state_dict
    sd = random_state_dict(384, 2, 14, 1 + 37 * 37, seed=0, well_conditioned=True)
    bb = ViTBackbone(sd, 14, DEV, dtype="float32")
    img = torch.randn(2, 3, 171, 300, generator=torch.Generator().manual_seed(1)).to(DEV)
    got = bb(img)
    assert got.shape == (2, 13, 22, 384)
    from dvt_amd.seg import center_pad
    (t, b), (l, r) = center_pad(171, 14), center_pad(300, 14)
    pad = torch.nn.functional.pad(img, (l, r, t, b))
    want = HipViT(sd, 14, 14, tuple(pad.shape[2:]), DEV, dtype="float32").forward_features(pad.contiguous())
    assert torch.equal(got, want)
    bb(torch.randn(1, 3, 512, 512, device=DEV))
    assert set(bb._engines) == {(182, 308), (518, 518)}
