"""GPU: `python -m dvt_amd.evaluate nyu_linear --task depth` end to end on a small synthetic NYU tree written here:
checkpoints with the reference's keys, eval_results.json with the nine metrics, the best-abs_rel checkpoint, resume across
iteration 100 bit for bit, the batch without a valid pixel, and the quality against the float64 restatement's training loop.

Quality (synthetic tree, random ViT-S, crop 112 x 140, 120 iterations, lr 0.01, warm-up 20): the yardstick's abs_rel over
the seeds 0, 1, 2 and the HIP run's at seed 0 are printed by the test; DESIGN section 9 records them."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

from tests import depth_reference as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
METRICS = ("a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel")


def write_nyu(root, n_train=6, n_val=3, seed=0, all_invalid=False):
    """480 x 640 JPEGs of smooth colour fields; the 16-bit depth (millimetres) is a smooth function of position and colour."""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, 480), np.linspace(0, 1, 640), indexing="ij")
    for split, n in (("train", n_train), ("test", n_val)):
        lines = []
        for i in range(n):
            a, b, c = rng.rand(3)
            r = 0.5 + 0.5 * np.sin(3 * xx + 6 * a)
            g = 0.5 + 0.5 * np.cos(2 * yy + 6 * b)
            bl = 0.5 + 0.5 * np.sin(2 * (xx + yy) + 6 * c)
            img = (np.stack([r, g, bl], -1) * 255).astype(np.uint8)
            depth = 1.0 + 3.0 * r + 2.0 * yy + 1.5 * g  # metres, 1 .. 7.5
            mm = (depth * 1000).astype(np.uint16)
            mm[:8] = 0  # the sensor's invalid border
            mm[:, :8] = 0
            if all_invalid:
                mm[:] = 0
            os.makedirs(os.path.join(root, split), exist_ok=True)
            Image.fromarray(img).save(os.path.join(root, split, f"rgb_{i:03d}.jpg"), quality=95)
            Image.fromarray(mm).save(os.path.join(root, split, f"depth_{i:03d}.png"))
            lines.append(f"/{split}/rgb_{i:03d}.jpg /{split}/depth_{i:03d}.png 518.86")
        lines.insert(1, f"/{split}/rgb_999.jpg None 518.86")
        with open(os.path.join(root, f"nyu_{split}.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


def run_eval(args, timeout=420):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "denoising-vit_amd"), ROOT, env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-m", "dvt_amd.evaluate", "nyu_linear", "--task", "depth", "--allow_random_vit",
                        "--launcher", "none", *args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


SHORT = ["crop_size=112,140", "lr_config.warmup_iters=20", "optimizer.lr=0.01", "log_config.interval=20"]
T = 120


@pytest.fixture(scope="module")
def nyu(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("nyu"))
    write_nyu(root)
    return root


@pytest.fixture(scope="module")
def full_run(nyu, tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("full"))
    out = run_eval(["--seed", "0", "--data-root", nyu, "--work-dir", wd, "--cfg-options", f"runner.max_iters={T}",
                    "checkpoint_config.interval=30", "evaluation.interval=60", *SHORT])
    return wd, out


def test_end_to_end_outputs(full_run):
    wd, out = full_run
    res = json.load(open(os.path.join(wd, "eval_results.json")))
    assert [r["iter"] for r in res] == [60, T]
    for r in res:
        assert set(r) == {"iter", *METRICS} and all(np.isfinite(r[k]) for k in METRICS)
    assert res[1]["abs_rel"] < res[0]["abs_rel"] or res[1]["abs_rel"] < 0.5
    ck = torch.load(os.path.join(wd, "latest.pth"), weights_only=False)
    assert set(ck) == {"meta", "state_dict", "optimizer"} and ck["meta"]["iter"] == T
    assert {k: tuple(v.shape) for k, v in ck["state_dict"].items()} == {
        "decode_head.conv_depth.weight": (256, 768, 1, 1), "decode_head.conv_depth.bias": (256,)}
    assert set(ck["optimizer"]["state"]) == {0, 1} and float(ck["optimizer"]["state"][0]["step"]) == T
    assert ck["optimizer"]["state"][0]["exp_avg"].shape == (256, 768)
    files = sorted(f for f in os.listdir(wd) if f.endswith(".pth"))
    assert [f for f in files if f.startswith("iter_")] == ["iter_120.pth", "iter_90.pth"]  # max_keep_ckpts = 2
    best = [f for f in files if f.startswith("best_abs_rel_iter_")]
    want_best = min(res, key=lambda r: r["abs_rel"])["iter"]
    assert best == [f"best_abs_rel_iter_{want_best}.pth"]
    assert "decode.loss_depth" in out and "decode.loss_grad: 0.0000" in out


def test_resume_across_iteration_100_is_bit_exact(nyu, full_run, tmp_path):
    wd, _ = full_run
    run_eval(["--seed", "0", "--data-root", nyu, "--work-dir", str(tmp_path), "--resume-from", os.path.join(wd, "iter_90.pth"),
              "--no-validate", "--cfg-options", f"runner.max_iters={T}", "checkpoint_config.interval=30", *SHORT])
    a = torch.load(os.path.join(wd, f"iter_{T}.pth"), weights_only=False)
    b = torch.load(os.path.join(str(tmp_path), f"iter_{T}.pth"), weights_only=False)
    for k, t in a["state_dict"].items():
        assert torch.equal(t, b["state_dict"][k]), k
    for i in (0, 1):
        for k in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(a["optimizer"]["state"][i][k], b["optimizer"]["state"][i][k]), (i, k)


def test_batches_without_a_valid_pixel_leave_the_parameters_untouched(tmp_path):
    from dvt_amd.depth import DepthHeadEngine
    root, wd = str(tmp_path / "nyu"), str(tmp_path / "wd")
    write_nyu(root, n_train=4, n_val=1, all_invalid=True)
    out = run_eval(["--seed", "3", "--data-root", root, "--work-dir", wd, "--no-validate", "--cfg-options", "runner.max_iters=3",
                    "checkpoint_config.interval=3", *SHORT])
    assert out.count("skipped: no valid ground-truth pixel") == 3
    ck = torch.load(os.path.join(wd, "iter_3.pth"), weights_only=False)
    fresh = DepthHeadEngine(384, DEV, seed=3).state_dict()
    for k, t in fresh.items():
        assert torch.equal(t, ck["state_dict"][k]), k
    assert ck["optimizer"]["state"] == {}


def test_quality_against_the_float64_training_loop(nyu, full_run):
    """The yardstick: the same data, seed, schedule and iteration count through tests/depth_reference.train_reference in
    float64 (its trained weights are scored by the HIP inference path, which test_gpu_depth_eval.py holds to 1e-5 of the
    restatement).  Margin: twice the spread of the yardstick's abs_rel over the seeds 0, 1, 2."""
    from dvt_amd import depth as DP
    from dvt_amd import depth_data as DD
    from dvt_amd import evaluate as E
    wd, _ = full_run
    cfg = E.build_depth_config("nyu_linear", [f"runner.max_iters={T}", *SHORT], nyu)
    args = types.SimpleNamespace(load_distilled_model_from=None, vit_checkpoint=None, load_denoiser_from=None, num_blocks=1,
                                 backbone_type="vit_small_patch14_dinov2.lvd142m", allow_random_vit=True, dtype="bfloat16")
    backbone, C = E.build_backbone(args, torch.device(DEV))
    backbone.return_cls = True
    train_ds = DD.NYUDataset(nyu, "nyu_train.txt")
    val_ds = DD.NYUDataset(nyu, "nyu_test.txt")
    opt, lrc = cfg["optimizer"], cfg["lr_config"]
    vals = {}
    for seed in (0, 1, 2):
        feeder = DD.DepthTrainFeeder(train_ds, 2, cfg["crop_size"], seed, 0, 1, 0, T, torch.device(DEV), workers=4)

        def sample(it):
            img, gt, _, _ = feeder.next()
            f, c = backbone(img)
            return f.cpu(), c.cpu(), gt.cpu()

        head = DP.DepthHeadEngine(C, DEV, seed=seed)
        v = head.views()
        try:
            W, b = ref.train_reference(sample, v["conv_depth.weight"].cpu(), v["conv_depth.bias"].cpu(), T,
                                       lambda it: DP.cosine_lr(it, opt["lr"], T, lrc["min_lr_ratio"], lrc["warmup_iters"], lrc["warmup_ratio"]),
                                       lambda it: DP.onecycle_beta1(it, T), weight_decay=opt["weight_decay"])
        finally:
            feeder.close()
        v["conv_depth.weight"].copy_(W.float())
        v["conv_depth.bias"].copy_(b.float())
        vals[seed] = DP.summarize(E.evaluate_depth(head, backbone, val_ds, cfg, 0, 1, torch.device(DEV)))["abs_rel"]
    hip = json.load(open(os.path.join(wd, "eval_results.json")))[-1]["abs_rel"]
    margin = 2 * (max(vals.values()) - min(vals.values()))
    print(f"abs_rel: HIP run (seed 0) {hip:.6f}; float64 yardstick seeds 0/1/2 {vals[0]:.6f} / {vals[1]:.6f} / {vals[2]:.6f}; margin {margin:.6f}")
    assert abs(hip - vals[0]) <= margin, (hip, vals, margin)
