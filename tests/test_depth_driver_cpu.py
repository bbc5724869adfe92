"""CPU: the `--task depth` side of `python -m dvt_amd.evaluate` and dvt_amd.depth_data: the nyu_linear preset against the
reference config's values (tests/golden/nyu_linear_reference_settings.json: numbers and names only), flags and
--cfg-options, every refusal by name, the task / config mismatch, the split parser, each transform against a direct numpy
statement with the order and count of its random draws, and the gathering of per-image metric rows over two gloo ranks."""
import json
import os

import numpy as np
import pytest
import torch

from dvt_amd import depth_data as DD
from dvt_amd import evaluate as E

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "nyu_linear_reference_settings.json")))


def norm(v):
    return json.loads(json.dumps(v, default=list))


def test_preset_matches_the_reference_settings():
    cfg = E.build_depth_config("nyu_linear")
    assert cfg["dataset_type"] == GOLD["dataset_type"] and list(cfg["crop_size"]) == GOLD["crop_size"]
    for k in ("samples_per_gpu", "workers_per_gpu", "train", "val"):
        assert norm(cfg["data"][k]) == GOLD["data"][k], k
    head = norm(cfg["model"]["decode_head"])
    for k, v in GOLD["decode_head"].items():
        if k not in ("in_channels", "channels"):  # set from the backbone here
            assert head[k] == v, k
    assert cfg["model"]["type"] == GOLD["model_type"] and cfg["model"]["test_cfg"] == GOLD["test_cfg"]
    for k in ("final_norm", "with_cls_token", "output_cls_token", "out_indices"):
        assert cfg["model"]["backbone"][k] == GOLD["backbone"][k]
    assert norm(cfg["optimizer"]) == GOLD["optimizer"]
    for k in ("lr_config", "momentum_config", "optimizer_config", "runner", "checkpoint_config", "evaluation"):
        assert norm(cfg[k]) == GOLD[k], k
    assert cfg["log_config"]["interval"] == GOLD["log_interval"]
    # no paramwise key matches decode_head.conv_depth.*: both tensors decay
    assert not any(key in name for key in GOLD["paramwise_custom_keys"]
                   for name in ("decode_head.conv_depth.weight", "decode_head.conv_depth.bias"))
    # the data constants of the pipeline
    assert list(DD.IMG_MEAN) == pytest.approx(GOLD["img_norm_cfg"]["mean"]) and list(DD.IMG_STD) == pytest.approx(GOLD["img_norm_cfg"]["std"])
    assert GOLD["train_pipeline"][2:8] == ["NYUCrop", "RandomRotate", "RandomFlip", "RandomCrop", "ColorAug", "Normalize"]
    assert GOLD["RandomRotate"] == {"prob": 0.5, "degree": 2.5} and GOLD["RandomFlip"] == {"prob": 0.5}
    assert GOLD["ColorAug"] == {"prob": 0.5, "gamma_range": [0.9, 1.1], "brightness_range": [0.75, 1.25], "color_range": [0.9, 1.1]}
    assert GOLD["test_img_scale"] == [480, 640] and GOLD["test_flip"] is True


def test_config_file_is_read_for_the_same_keys(tmp_path):
    path = tmp_path / "nyu_cfg.py"
    path.write_text(
        "dataset_type = 'NYUDataset'\ncrop_size = (320, 416)\n"
        "train_pipeline = [dict(type='NYUCrop', depth=True), dict(type='RandomCrop', crop_size=crop_size)]\n"
        "data = dict(samples_per_gpu=4, train=dict(type=dataset_type, data_root='d', depth_scale=1000, split='a.txt',"
        " pipeline=train_pipeline, eigen_crop=True, min_depth=0.001, max_depth=10),"
        " val=dict(type=dataset_type, data_root='d', depth_scale=1000, split='b.txt', eigen_crop=True))\n"
        "model = dict(type='DepthEncoderDecoder', backbone=dict(type='DinoVisionTransformer', out_indices=[11]),"
        " decode_head=dict(type='BNHead', norm_cfg=None, classify=True, n_bins=128, bins_strategy='UD', norm_strategy='linear',"
        " upsample=4, loss_decode=[dict(type='SigLoss', valid_mask=True, loss_weight=1.0, warm_up=True),"
        " dict(type='GradientLoss', valid_mask=True, loss_weight=0.5)]), test_cfg=dict(mode='whole'))\n"
        "optimizer = dict(type='AdamW', lr=0.001, betas=(0.9, 0.999), weight_decay=0.01, paramwise_cfg=dict(custom_keys=dict()))\n"
        "lr_config = dict(policy='CosineAnnealing', warmup='linear', warmup_iters=10, warmup_ratio=0.001, min_lr_ratio=1e-08, by_epoch=False)\n"
        "runner = dict(type='IterBasedRunner', max_iters=100)\n")
    assert E.config_kind(str(path)) == "depth"
    cfg = E.build_depth_config(str(path), ["runner.max_iters=50"], data_root="/x")
    assert cfg["crop_size"] == (320, 416) and cfg["data"]["samples_per_gpu"] == 4 and cfg["runner"]["max_iters"] == 50
    assert cfg["model"]["decode_head"]["n_bins"] == 128 and cfg["optimizer"]["lr"] == 0.001
    assert cfg["data"]["train"]["data_root"] == "/x" and cfg["data"]["val"]["split"] == "b.txt"
    assert E.get_args([str(path), "--task", "depth"]).task == "depth"
    with pytest.raises(SystemExit):
        E.get_args([str(path)])


def test_flags_and_cfg_options():
    a = E.get_args(["nyu_linear", "--task", "depth", "--data-root", "data/nyu", "--no-validate", "--auto-resume",
                    "--resume-from", "x.pth", "--cfg-options", "runner.max_iters=10", "data.samples_per_gpu=3"])
    assert a.task == "depth" and a.no_validate and a.auto_resume and a.resume_from == "x.pth"
    cfg = E.build_depth_config("nyu_linear", a.cfg_options, a.data_root)
    assert cfg["runner"]["max_iters"] == 10 and cfg["data"]["samples_per_gpu"] == 3


@pytest.mark.parametrize("argv,kind", [(["voc2012_linear", "--task", "depth"], "segmentation"), (["ade20k_linear", "--task", "depth"], "segmentation"),
                                       (["nyu_linear"], "depth"), (["nyu_linear", "--task", "segmentation"], "depth")])
def test_task_and_config_must_match(argv, kind, capsys):
    with pytest.raises(SystemExit):
        E.get_args(argv)
    err = capsys.readouterr().err
    assert f"is a {kind} config, not a" in err


@pytest.mark.parametrize("option,name", [
    ("model.decode_head.type=DPTHead", "DPTHead"), ("model.decode_head.classify=False", "classify=False"),
    ("model.decode_head.bins_strategy=SID", "bins_strategy=SID"), ("model.decode_head.norm_strategy=softmax", "norm_strategy=softmax"),
    ("model.decode_head.norm_strategy=sigmoid", "norm_strategy=sigmoid"), ("model.decode_head.scale_up=True", "scale_up"),
    ("model.test_cfg.mode=slide", "mode=slide"), ("data.train.type=KITTIDataset", "KITTIDataset"),
    ("data.val.garg_crop=True", "garg_crop"), ("optimizer.type=SGD", "SGD"), ("lr_config.policy=poly", "policy=poly"),
    ("momentum_config.policy=cyclic", "cyclic"), ("model.decode_head.align_corners=True", "align_corners"),
    ("model.backbone.out_indices=[8,9,10,11]", "out_indices"), ("model.decode_head.upsample=16", "upsample=16"),
    ("model.decode_head.norm_cfg.type=SyncBN", "norm_cfg"), ("runner.type=EpochBasedRunner", "EpochBasedRunner"),
    ("optimizer_config.grad_clip.norm_type=1", "norm_type=1"), ("lr_config.by_epoch=True", "by_epoch"),
    ("model.type=EncoderDecoder", "model.type=EncoderDecoder")])
def test_refusals_name_the_value(option, name):
    with pytest.raises(NotImplementedError) as e:
        E.build_depth_config("nyu_linear", [option])
    assert name in str(e.value) and "not supported" in str(e.value)


def test_other_losses_are_refused():
    cfg_opt = ["model.decode_head.loss_decode.0.type=L1"]  # a dict-keyed override does not match the list: build by hand
    import copy
    cfg = copy.deepcopy(E.DEPTH_PRESETS["nyu_linear"])
    cfg["model"]["decode_head"]["loss_decode"] = [{"type": "SigLoss", "valid_mask": True, "warm_up": True}]
    with pytest.raises(NotImplementedError) as e:
        E.validate_depth(cfg)
    assert "loss_decode" in str(e.value)
    del cfg_opt


def test_split_parser(tmp_path):
    text = "/b/rgb_2.jpg /b/d_2.png 518.8\na/rgb_1.jpg a/d_1.png 518.8\nc/rgb_3.jpg None 518.8\n\n"
    got = DD.parse_split(text, "/root_dir")
    assert got == [("/root_dir/a/rgb_1.jpg", "/root_dir/a/d_1.png"), ("/root_dir/b/rgb_2.jpg", "/root_dir/b/d_2.png")]
    (tmp_path / "s.txt").write_text(text)
    assert len(DD.NYUDataset(str(tmp_path), "s.txt")) == 2


class CountingRng:
    """Records the calls made on a RandomState."""

    def __init__(self, seed):
        self.r, self.calls = np.random.RandomState(seed), []

    def rand(self):
        self.calls.append("rand")
        return self.r.rand()

    def uniform(self, lo, hi, size=None):
        self.calls.append(("uniform", lo, hi, size))
        return self.r.uniform(lo, hi, size)

    def randint(self, lo, hi):
        self.calls.append(("randint", lo, hi))
        return self.r.randint(lo, hi)


def test_train_sample_draw_order_and_count():
    img = np.random.RandomState(0).randint(0, 256, (480, 640, 3)).astype(np.uint8)
    depth = np.random.RandomState(1).rand(480, 640).astype(np.float32) * 9
    for seed in range(6):
        rng = CountingRng(seed)
        DD.train_sample(img, depth, rng)
        c = rng.calls
        # rotate: decision + angle ALWAYS; flip; crop y then x; colour decision (+ gamma, brightness, three colours)
        assert c[:6] == ["rand", ("uniform", -2.5, 2.5, None), "rand", ("randint", 0, 427 - 416 + 1), ("randint", 0, 565 - 544 + 1), "rand"]
        assert c[6:] in ([], [("uniform", 0.9, 1.1, None), ("uniform", 0.75, 1.25, None), ("uniform", 0.9, 1.1, 3)])
    seen = {len(CountingRngRun(s)) for s in range(12)}
    assert seen == {6, 9}


def CountingRngRun(seed):
    rng = CountingRng(seed)
    DD.train_sample(np.zeros((480, 640, 3), np.uint8), np.zeros((480, 640), np.float32), rng)
    return rng.calls


def test_rotate_angle_is_drawn_even_when_not_rotating():
    class Fixed(CountingRng):
        def rand(self):
            self.calls.append("rand")
            return 0.9  # no rotation
    rng = Fixed(0)
    img, depth = np.arange(5 * 6 * 3, dtype=np.uint8).reshape(5, 6, 3), np.arange(30, dtype=np.float32).reshape(5, 6)
    i2, d2 = DD.random_rotate(img, depth, rng)
    assert rng.calls == ["rand", ("uniform", -2.5, 2.5, None)] and i2 is img and d2 is depth


def test_nyu_crop_flip_and_random_crop():
    img = np.random.RandomState(0).randint(0, 256, (480, 640, 3)).astype(np.uint8)
    depth = np.random.RandomState(1).rand(480, 640).astype(np.float32)
    i, d = DD.nyu_crop(img, depth)
    assert i.shape == (427, 565, 3) and np.array_equal(i, img[45:472, 43:608]) and np.array_equal(d, depth[45:472, 43:608])
    rng = np.random.RandomState(3)
    want = np.random.RandomState(3)
    ci, cd = DD.random_crop(i, d, rng)
    oy = want.randint(0, 12)
    ox = want.randint(0, 22)
    assert np.array_equal(ci, i[oy:oy + 416, ox:ox + 544]) and np.array_equal(cd, d[oy:oy + 416, ox:ox + 544])

    class Always:
        def rand(self):
            return 0.1
    fi, fd = DD.random_flip(i, d, Always())
    assert np.array_equal(fi, i[:, ::-1]) and np.array_equal(fd, d[:, ::-1])


def test_rotate_against_a_direct_statement():
    rs = np.random.RandomState(0)
    img = rs.randint(0, 256, (9, 11, 3)).astype(np.uint8)
    depth = rs.rand(9, 11).astype(np.float32) * 5
    assert np.array_equal(DD.rotate(img, 0.0, False), img) and np.array_equal(DD.rotate(depth, 0.0, True), depth)
    # 180 degrees about ((w - 1) / 2, (h - 1) / 2) is the point reflection
    assert np.array_equal(DD.rotate(depth, 180.0, True), depth[::-1, ::-1])
    assert np.abs(DD.rotate(img, 180.0, False).astype(int) - img[::-1, ::-1].astype(int)).max() <= 1
    # a small angle, pixel by pixel: inverse map, positive angle = clockwise
    ang = 2.0
    a = np.deg2rad(-ang)
    got_i, got_d = DD.rotate(img, ang, False), DD.rotate(depth, ang, True)
    h, w = depth.shape
    cx, cy = (w - 1) / 2, (h - 1) / 2
    for (y, x) in [(0, 0), (4, 5), (8, 10), (2, 9), (7, 1)]:
        sx = np.cos(a) * (x - cx) - np.sin(a) * (y - cy) + cx
        sy = np.sin(a) * (x - cx) + np.cos(a) * (y - cy) + cy
        ny, nx = int(np.floor(sy + 0.5)), int(np.floor(sx + 0.5))
        want_d = depth[ny, nx] if 0 <= ny < h and 0 <= nx < w else 0.0
        assert got_d[y, x] == want_d
        x0, y0 = int(np.floor(sx)), int(np.floor(sy))
        acc = np.zeros(3)
        for yy, wy in ((y0, 1 - (sy - y0)), (y0 + 1, sy - y0)):
            for xx, wx in ((x0, 1 - (sx - x0)), (x0 + 1, sx - x0)):
                if 0 <= yy < h and 0 <= xx < w:
                    acc += wy * wx * img[yy, xx]
        assert np.array_equal(got_i[y, x], np.clip(np.rint(acc), 0, 255).astype(np.uint8))


def test_color_aug_is_on_the_0_255_scale_in_bgr_order():
    img = np.random.RandomState(0).randint(1, 256, (4, 5, 3)).astype(np.uint8)
    rng = np.random.RandomState(5)
    while True:  # a seed state whose first draw applies the augmentation
        state = rng.get_state()
        if rng.rand() < 0.5:
            break
    rng.set_state(state)
    want = np.random.RandomState()
    want.set_state(state)
    got = DD.color_aug(img, rng)
    want.rand()
    gamma = want.uniform(0.9, 1.1)
    bright = want.uniform(0.75, 1.25)
    colors = want.uniform(0.9, 1.1, size=3)
    bgr = img[:, :, ::-1].astype(np.float64)  # as the reference holds the image
    exp = np.clip(bgr ** gamma * bright * colors[None, None, :], 0, 255)[:, :, ::-1]
    assert np.allclose(got, exp, rtol=1e-12, atol=0)
    assert got.max() > 1.5  # 0-255 values, not 0-1
    assert not np.allclose(got, np.clip(img.astype(np.float64) ** gamma * bright * colors[None, None, :], 0, 255))

    class Never:
        def rand(self):
            return 0.7
    assert DD.color_aug(img, Never()) is img


def test_normalize_and_samples():
    img = np.random.RandomState(0).randint(0, 256, (480, 640, 3)).astype(np.uint8)
    depth = (np.random.RandomState(1).rand(480, 640) * 9).astype(np.float32)
    x = DD.test_sample(img)
    assert x.shape == (3, 480, 640) and x.dtype == np.float32
    assert np.allclose(x[1], (img[:, :, 1].astype(np.float32) - 116.28) / 57.12, atol=1e-6)
    im, dp = DD.train_sample(img, depth, np.random.RandomState(2))
    assert im.shape == (3, 416, 544) and dp.shape == (416, 544) and dp.dtype == np.float32 and im.dtype == np.float32


def _gather_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    n = 5
    full = torch.arange(n * 9, dtype=torch.float64).reshape(n, 9)
    full[3] = float("nan")
    got = E.gather_metric_rows(full[rank::world].clone(), n, rank, world)
    ok = torch.equal(torch.nan_to_num(got, nan=-1.0), torch.nan_to_num(full, nan=-1.0))
    torch.save(ok, os.path.join(out, f"ok{rank}.pt"))
    dist.destroy_process_group()


def test_metric_rows_gather_over_two_gloo_ranks(tmp_path):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_gather_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert all(torch.load(tmp_path / f"ok{r}.pt") for r in range(2))
    one = torch.arange(18, dtype=torch.float64).reshape(2, 9)
    assert E.gather_metric_rows(one, 2, 0, 1) is one
