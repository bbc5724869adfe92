"""CPU: the segmentation-evaluation driver (dvt_amd.evaluate) and data pipeline (dvt_amd.seg_data) -- flag parity with
the reference's parser, presets, --cfg-options, refusals, mmcv / mmseg transform rules, rank sharding."""
import json
import os

import numpy as np
import pytest

from dvt_amd import evaluate as E
from dvt_amd import seg_data as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_dense_reference_flags.json")


def test_every_reference_flag_is_accepted():
    flags = json.load(open(GOLDEN))["flags"]
    p = E.get_args.__code__  # noqa: F841  (the parser is built inside get_args)
    import argparse
    seen = set()
    orig = argparse.ArgumentParser.add_argument

    def spy(self, *names, **kw):
        seen.update(n.lstrip("-") for n in names)
        return orig(self, *names, **kw)

    argparse.ArgumentParser.add_argument = spy
    try:
        E.get_args(["voc2012_linear"])
    finally:
        argparse.ArgumentParser.add_argument = orig
    assert set(flags) <= seen, sorted(set(flags) - seen)


@pytest.mark.parametrize("argv", [["voc2012_linear", "--task", "depth"], ["voc2012_linear", "--launcher", "slurm"],
                                  ["voc2012_linear", "--launcher", "mpi"]])
def test_unsupported_task_and_launchers_are_refused(argv, capsys):
    with pytest.raises(SystemExit):
        E.get_args(argv)
    assert "not" in capsys.readouterr().err


def test_presets():
    for name, K, ds in (("voc2012_linear", 21, "PascalVOCDataset"), ("ade20k_linear", 150, "ADE20KDataset")):
        c = E.build_config(name)
        assert c["runner"]["max_iters"] == 40000 and c["data"]["samples_per_gpu"] == 2
        assert c["checkpoint_config"]["interval"] == 10000 and c["evaluation"]["interval"] == 10000
        assert c["optimizer"] == {"type": "AdamW", "lr": 1e-3, "weight_decay": 1e-4, "betas": (0.9, 0.999)}
        lr = c["lr_config"]
        assert (lr["policy"], lr["warmup"], lr["warmup_iters"], lr["warmup_ratio"], lr["power"], lr["min_lr"]) == \
            ("poly", "linear", 1500, 1e-6, 1.0, 0.0)
        assert c["model"]["test_cfg"] == {"mode": "slide", "crop_size": (512, 512), "stride": (341, 341)}
        assert c["model"]["decode_head"]["num_classes"] == K and c["data"]["train"]["type"] == ds


def test_cfg_options():
    c = E.build_config("voc2012_linear", ["runner.max_iters=300", "optimizer.lr=0.01", "evaluation.interval=100",
                                          "model.test_cfg.stride=(256,256)", "data.samples_per_gpu=4"])
    assert c["runner"]["max_iters"] == 300 and c["optimizer"]["lr"] == 0.01
    assert c["model"]["test_cfg"]["stride"] == (256, 256) and c["data"]["samples_per_gpu"] == 4
    assert E.parse_value("a,b") == ["a", "b"] and E.parse_value("True") is True and E.parse_value("x") == "x"


@pytest.mark.parametrize("opt,name", [
    ("model.decode_head.type=FCNHead", "decode_head.type"),
    ("model.decode_head.input_transform=multiple_select", "input_transform"),
    ("model.decode_head.in_index=[0,1,2,3]", "in_index"),
    ("model.decode_head.loss_decode.type=FocalLoss", "loss_decode"),
    ("model.test_cfg.mode=whole", "test_cfg.mode"),
    ("data.train.type=CityscapesDataset", "data.train.type"),
    ("optimizer.type=SGD", "optimizer.type"),
])
def test_unsupported_config_values_are_refused(opt, name):
    with pytest.raises(NotImplementedError, match=name.replace(".", r"\.")):
        E.build_config("voc2012_linear", [opt])


def test_reference_style_config_file(tmp_path):
    p = tmp_path / "cfg.py"
    p.write_text('dataset_type = "ADE20KDataset"\ndata_root = "d"\nnum_classes = 150\ncrop_size = (512, 512)\n'
                 'data = dict(samples_per_gpu=2, train=dict(type=dataset_type, data_root=data_root, img_dir="i", '
                 'ann_dir="a", pipeline=[dict(type="RandomCrop", crop_size=crop_size, cat_max_ratio=0.75)]), '
                 'val=dict(type=dataset_type, data_root=data_root, img_dir="iv", ann_dir="av"))\n'
                 'optimizer = dict(type="AdamW", lr=0.001, weight_decay=0.0001, betas=(0.9, 0.999))\n'
                 'runner = dict(type="IterBasedRunner", max_iters=40000)\n'
                 'model = dict(type="EncoderDecoder", decode_head=dict(type="BNHead", in_index=[3], '
                 'num_classes=num_classes), test_cfg=dict(mode="slide", crop_size=(512, 512), stride=(341, 341)))\n')
    c = E.build_config(str(p))
    assert c["model"]["decode_head"]["num_classes"] == 150 and c["data"]["train"]["img_dir"] == "i"
    p.write_text(p.read_text().replace('type="BNHead"', 'type="DPTHead"'))
    with pytest.raises(NotImplementedError, match="DPTHead"):
        E.build_config(str(p))


def test_rescale_size():
    # mmcv.rescale_size(old (w, h), (2048, 512)): factor min(2048 / long, 512 / short), rounded half up
    assert D.rescale_size(500, 375, (2048, 512)) == (683, 512)
    assert D.rescale_size(2000, 300, (2048, 512)) == (2048, 307)
    assert D.rescale_size(500, 375, (1024, 256)) == (341, 256)


def test_random_crop_redraws_until_no_class_dominates():
    lab = np.zeros((600, 600), np.uint8)
    lab[:, 550:] = 1  # only crops reaching x >= 550 see a second class at all
    rng = np.random.RandomState(0)
    draws = []

    class Spy:
        def randint(self, lo, hi):
            v = rng.randint(lo, hi)
            draws.append(v)
            return v
    box = D.random_crop_bbox(lab, (512, 512), 0.75, Spy())
    n = len(draws) // 2
    assert 1 <= n <= 11
    y1, y2, x1, x2 = box
    labels, cnt = np.unique(lab[y1:y2, x1:x2], return_counts=True)
    if n < 11:  # stopped early: the crop passes the test
        assert len(cnt) > 1 and cnt.max() / cnt.sum() < 0.75
    # a label that is all one class redraws ten times and keeps the last box
    draws.clear()
    D.random_crop_bbox(np.zeros((600, 600), np.uint8), (512, 512), 0.75, Spy())
    assert len(draws) == 22
    # ignored pixels do not count
    lab2 = np.full((512, 512), 255, np.uint8)
    lab2[:10] = 1
    lab2[10:30] = 2
    draws.clear()
    D.random_crop_bbox(lab2, (512, 512), 0.75, Spy())
    assert len(draws) == 2


def test_pad_bottom_right():
    img = np.ones((300, 400, 3), np.float32)
    lab = np.zeros((300, 400), np.uint8)
    pi, pl = D.pad(img, lab, (512, 512))
    assert pi.shape == (512, 512, 3) and pl.shape == (512, 512)
    assert pi[:300, :400].min() == 1 and pi[300:].max() == 0 and pi[:, 400:].max() == 0
    assert (pl[300:] == 255).all() and (pl[:, 400:] == 255).all() and (pl[:300, :400] == 0).all()


def test_train_sample_shapes_and_reduce_zero_label():
    rng = np.random.RandomState(1)
    img = rng.randint(0, 255, (120, 90, 3)).astype(np.uint8)
    lab = rng.randint(0, 3, (120, 90)).astype(np.uint8)
    x, y = D.train_sample(img, lab, np.random.RandomState(3))
    assert x.shape == (3, 512, 512) and y.shape == (512, 512) and x.dtype == np.float32
    assert D.reduce_zero_label(np.array([0, 1, 2, 150, 255], np.uint8)).tolist() == [255, 0, 1, 149, 255]
    h = D.rgb_to_hsv(img)
    assert h[..., 0].max() < 180
    assert np.abs(D.hsv_to_rgb(h).astype(int) - img).max() <= 5  # H kept in 2-degree steps


def test_rank_sharding_covers_each_epoch_once():
    n, B, world = 11, 2, 2
    per_epoch = -(-n // world) // B
    seen = []
    for it in range(per_epoch):
        for r in range(world):
            seen += D.batch_indices(n, it, B, 5, r, world)
    assert len(seen) == per_epoch * B * world == 12
    assert set(seen) == set(range(n))  # DistributedSampler pads 11 to 12 by repeating the permutation's head
    assert D.batch_indices(n, 3, B, 5, 0, world) == D.batch_indices(n, 3, B, 5, 0, world)
    assert D.batch_indices(n, per_epoch, B, 5, 0, 1) != D.batch_indices(n, 0, B, 5, 0, 1) or n < 3
