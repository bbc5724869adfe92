"""`python -m dvt_amd.evaluate`: the reference's `evaluate_dense_tasks.py --task segmentation` with the linear configs.

A linear probe (mmseg 0.27's BNHead: SyncBN + conv_seg) is trained on the frozen features of a DINOv2 ViT, a stage-2
`Denoiser` on top of it (--load-denoiser-from) or a distilled ViT (--load-distilled-model-from), then evaluated by slide
inference: mIoU / mAcc / aAcc on PascalVOC 2012 or ADE20K.  The head runs on csrc/dvt_seg.hip (dvt_amd.seg), the backbone
on the HIP extractor, the data pipeline on host threads (dvt_amd.seg_data).

`config` is a preset (`voc2012_linear`, `ade20k_linear`) or a reference-style config file; the keys the port reads are
listed in `PRESETS`, anything it does not implement is refused by name.  Multi-GPU: `torchrun --nproc_per_node N -m
dvt_amd.evaluate ...` (launcher pytorch): rank sharding of a seeded per-epoch permutation, SyncBN by merging the ranks'
statistics records, one flat gradient all-reduce per step, evaluation histograms all-reduced with SUM.

Outputs in --work-dir: iter_{n}.pth / latest.pth (mmcv layout: meta, state_dict, optimizer), a log with mmseg's per-class
table, and eval_results.json.

`--task depth` with the `nyu_linear` preset (or a reference-style depth config file) is the reference's NYU Depth v2 linear
probe: the depth BNHead on csrc/dvt_depth.hip (dvt_amd.depth) over the patch tokens and the cls token, the data pipeline of
dvt_amd.depth_data, flip-averaged whole-image inference and the nine metrics; besides the files above it keeps the newest
two iter_{n}.pth and best_abs_rel_iter_{n}.pth.  A task that does not match the config's kind is refused.
"""
from __future__ import annotations

import argparse
import ast
import copy
import json
import os
import random
import shutil
import time

import numpy as np
import torch

from . import arena
from . import depth as DP
from . import depth_data as DD
from . import seg as S
from . import seg_data as D


def _common(dataset_type, data_root, num_classes, train_dirs, val_dirs):
    return {
        "dataset_type": dataset_type,
        "data": {"samples_per_gpu": 2, "workers_per_gpu": 4,
                 "train": {"type": dataset_type, "data_root": data_root, **train_dirs},
                 "val": {"type": dataset_type, "data_root": data_root, **val_dirs}},
        "crop_size": (512, 512),
        "img_scale": (2048, 512),
        "optimizer": {"type": "AdamW", "lr": 1e-3, "weight_decay": 1e-4, "betas": (0.9, 0.999)},
        "lr_config": {"policy": "poly", "warmup": "linear", "warmup_iters": 1500, "warmup_ratio": 1e-6, "power": 1.0,
                      "min_lr": 0.0, "by_epoch": False},
        "runner": {"type": "IterBasedRunner", "max_iters": 40000},
        "checkpoint_config": {"by_epoch": False, "interval": 10000},
        "evaluation": {"interval": 10000, "metric": "mIoU"},
        "log_config": {"interval": 50},
        "model": {"type": "EncoderDecoder", "backbone": {"out_indices": [8, 9, 10, 11]},
                  "decode_head": {"type": "BNHead", "in_index": [3], "input_transform": "resize_concat",
                                  "num_classes": num_classes, "align_corners": False, "dropout_ratio": 0,
                                  "loss_decode": {"type": "CrossEntropyLoss", "use_sigmoid": False, "loss_weight": 1.0}},
                  "test_cfg": {"mode": "slide", "crop_size": (512, 512), "stride": (341, 341)}},
        "work_dir": None,
    }


PRESETS = {
    "voc2012_linear": _common("PascalVOCDataset", "data/VOCdevkit/VOC2012", 21,
                              {"img_dir": "JPEGImages", "ann_dir": "SegmentationClass",
                               "split": "ImageSets/Segmentation/train.txt"},
                              {"img_dir": "JPEGImages", "ann_dir": "SegmentationClass",
                               "split": "ImageSets/Segmentation/val.txt"}),
    "ade20k_linear": _common("ADE20KDataset", "data/ADEChallengeData2016", 150,
                             {"img_dir": "images/training", "ann_dir": "annotations/training"},
                             {"img_dir": "images/validation", "ann_dir": "annotations/validation"}),
}


def _nyu_part(split):
    return {"type": "NYUDataset", "data_root": "data/nyu", "depth_scale": 1000, "split": split, "garg_crop": False,
            "eigen_crop": True, "min_depth": 0.001, "max_depth": 10}


# the values of the reference's vitb_nyu_linear_config.py that the port reads
DEPTH_PRESETS = {
    "nyu_linear": {
        "dataset_type": "NYUDataset",
        "data": {"samples_per_gpu": 2, "workers_per_gpu": 2, "train": _nyu_part("nyu_train.txt"), "val": _nyu_part("nyu_test.txt")},
        "crop_size": (416, 544),
        "optimizer": {"type": "AdamW", "lr": 0.005, "betas": (0.9, 0.999), "weight_decay": 0.01},
        "lr_config": {"policy": "CosineAnnealing", "warmup": "linear", "warmup_iters": 12800, "warmup_ratio": 0.001,
                      "min_lr_ratio": 1e-8, "by_epoch": False},
        "momentum_config": {"policy": "OneCycle"},
        "optimizer_config": {"grad_clip": {"max_norm": 35, "norm_type": 2}},
        "runner": {"type": "IterBasedRunner", "max_iters": 38400},
        "checkpoint_config": {"by_epoch": False, "max_keep_ckpts": 2, "interval": 1600},
        "evaluation": {"by_epoch": False, "interval": 800, "pre_eval": True, "rule": "less", "save_best": "abs_rel"},
        "log_config": {"interval": 50},
        "model": {"type": "DepthEncoderDecoder",
                  "backbone": {"final_norm": True, "with_cls_token": True, "output_cls_token": True, "out_indices": [11]},
                  "decode_head": {"type": "BNHead", "norm_cfg": None, "min_depth": 0.001, "max_depth": 10,
                                  "loss_decode": [{"type": "SigLoss", "valid_mask": True, "loss_weight": 1.0, "warm_up": True,
                                                   "loss_name": "loss_depth"},
                                                  {"type": "GradientLoss", "valid_mask": True, "loss_weight": 0.5,
                                                   "loss_name": "loss_grad"}],
                                  "classify": True, "n_bins": 256, "bins_strategy": "UD", "norm_strategy": "linear",
                                  "upsample": 4, "in_index": [0], "input_transform": "resize_concat", "align_corners": False},
                  "test_cfg": {"mode": "whole"}},
        "work_dir": None,
    },
}


# ================================================================================================ configuration
def _merge(dst: dict, src: dict) -> None:
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            _merge(dst[k], v)
        else:
            dst[k] = v


def load_config_file(path: str) -> dict:
    """Read a reference-style (mmcv) config file: its top-level assignments, evaluated as Python literals and dict(...)
    calls, with names bound earlier in the file.  `custom_imports` and `_base_` are not followed."""
    tree = ast.parse(open(path).read(), path)
    env: dict = {}

    def ev(node):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "dict" and not node.args:
            out = {}
            for kw in node.keywords:
                if kw.arg is None:
                    out.update(ev(kw.value))
                else:
                    out[kw.arg] = ev(kw.value)
            return out
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "range":
            return list(range(*[ev(a) for a in node.args]))
        if isinstance(node, ast.Name):
            if node.id in env:
                return copy.deepcopy(env[node.id])
            if node.id in ("True", "False", "None"):
                return {"True": True, "False": False, "None": None}[node.id]
            raise ValueError(f"{path}: unknown name {node.id}")
        if isinstance(node, ast.Dict):
            return {ev(k): ev(v) for k, v in zip(node.keys, node.values)}
        if isinstance(node, (ast.List, ast.Tuple)):
            vals = [ev(e) for e in node.elts]
            return vals if isinstance(node, ast.List) else tuple(vals)
        return ast.literal_eval(node)

    for stmt in tree.body:
        if isinstance(stmt, ast.Assign) and len(stmt.targets) == 1 and isinstance(stmt.targets[0], ast.Name):
            env[stmt.targets[0].id] = ev(stmt.value)
    return env


def from_file(path: str) -> dict:
    raw = load_config_file(path)
    data = raw.get("data", {})
    train, val = data.get("train", {}), data.get("val", {})
    ds_type = train.get("type", raw.get("dataset_type"))
    K = raw.get("model", {}).get("decode_head", {}).get("num_classes", 21)
    cfg = _common(ds_type, train.get("data_root", ""), K, {}, {})
    for part in ("train", "val"):
        src = data.get(part, {})
        cfg["data"][part] = {k: src[k] for k in ("type", "data_root", "img_dir", "ann_dir", "split") if k in src}
    for k in ("samples_per_gpu", "workers_per_gpu"):
        if k in data:
            cfg["data"][k] = data[k]
    for k in ("optimizer", "lr_config", "runner", "checkpoint_config", "evaluation", "log_config", "work_dir"):
        if k in raw:
            cfg[k] = raw[k]
    m = raw.get("model", {})
    cfg["model"] = {"type": m.get("type"), "backbone": m.get("backbone", {}), "decode_head": m.get("decode_head", {}),
                    "test_cfg": m.get("test_cfg", {})}
    for p in train.get("pipeline", []):
        if p.get("type") == "RandomCrop":
            cfg["crop_size"] = tuple(p["crop_size"])
        if p.get("type") == "Resize" and "img_scale" in p:
            cfg["img_scale"] = tuple(p["img_scale"])
    return cfg


def from_file_depth(path: str) -> dict:
    raw = load_config_file(path)
    cfg = copy.deepcopy(DEPTH_PRESETS["nyu_linear"])
    data = raw.get("data", {})
    for part in ("train", "val"):
        if part in data:
            cfg["data"][part] = {k: v for k, v in data[part].items() if k != "pipeline"}
    for k in ("samples_per_gpu", "workers_per_gpu"):
        if k in data:
            cfg["data"][k] = data[k]
    for k in ("dataset_type", "optimizer", "lr_config", "momentum_config", "optimizer_config", "runner", "checkpoint_config",
              "evaluation", "log_config", "work_dir"):
        if k in raw:
            cfg[k] = raw[k]
    cfg["optimizer"] = {k: v for k, v in cfg["optimizer"].items() if k != "paramwise_cfg"}  # no key of it matches the head
    m = raw.get("model", {})
    cfg["model"] = {"type": m.get("type"), "backbone": m.get("backbone", {}), "decode_head": m.get("decode_head", {}),
                    "test_cfg": m.get("test_cfg", {})}
    cfg["model"]["backbone"].pop("type", None)
    for p in data.get("train", {}).get("pipeline", []):
        if p.get("type") == "RandomCrop":
            cfg["crop_size"] = tuple(p["crop_size"])
    return cfg


def config_kind(config: str) -> str:
    """"depth" or "segmentation": what a preset or a config file describes."""
    if config in DEPTH_PRESETS:
        return "depth"
    if config in PRESETS or not os.path.exists(config):
        return "segmentation"
    raw = load_config_file(config)
    depth = raw.get("model", {}).get("type") == "DepthEncoderDecoder" or raw.get("dataset_type") in ("NYUDataset", "KITTIDataset")
    return "depth" if depth else "segmentation"


def validate_depth(cfg: dict) -> None:
    """Refuse what the depth port does not implement, naming the value."""
    def need(cond, what):
        if not cond:
            raise NotImplementedError(f"not supported by this port: {what}")
    m = cfg["model"]
    head = m.get("decode_head", {})
    need(m.get("type", "DepthEncoderDecoder") == "DepthEncoderDecoder", f"model.type={m.get('type')}")
    need(head.get("type", "BNHead") == "BNHead", f"model.decode_head.type={head.get('type')}")
    need(head.get("norm_cfg") is None, f"model.decode_head.norm_cfg={head.get('norm_cfg')}")
    need(head.get("classify", True), "model.decode_head.classify=False")
    need(head.get("bins_strategy", "UD") == "UD", f"model.decode_head.bins_strategy={head.get('bins_strategy')}")
    need(head.get("norm_strategy", "linear") == "linear", f"model.decode_head.norm_strategy={head.get('norm_strategy')}")
    need(not head.get("scale_up", False), "model.decode_head.scale_up=True")
    need(head.get("input_transform", "resize_concat") == "resize_concat",
         f"model.decode_head.input_transform={head.get('input_transform')}")
    need(len(head.get("in_index", [0])) == 1, f"model.decode_head.in_index={head.get('in_index')} (one layer only)")
    need(len(m.get("backbone", {}).get("out_indices", [11])) == 1,
         f"model.backbone.out_indices={m.get('backbone', {}).get('out_indices')} (the last block only)")
    need(m.get("backbone", {}).get("final_norm", True) and m.get("backbone", {}).get("output_cls_token", True),
         "model.backbone without final_norm / output_cls_token")
    need(not head.get("align_corners", False), "model.decode_head.align_corners=True")
    need(1 <= int(head.get("upsample", 4)) <= 8, f"model.decode_head.upsample={head.get('upsample')}")
    nb = head.get("n_bins", 256)
    need(isinstance(nb, int) and 4 <= nb <= 256 and nb % 4 == 0, f"model.decode_head.n_bins={nb}")
    losses = head.get("loss_decode", [])
    losses = losses if isinstance(losses, (list, tuple)) else [losses]
    ok = (len(losses) == 2 and losses[0].get("type") == "SigLoss" and losses[0].get("valid_mask", True)
          and losses[0].get("warm_up", False) and losses[0].get("loss_weight", 1.0) == 1.0
          and losses[0].get("warm_iter", 100) == 100 and losses[0].get("max_depth") is None
          and losses[1].get("type") == "GradientLoss" and losses[1].get("valid_mask", True)
          and losses[1].get("max_depth") is None)
    need(ok, f"model.decode_head.loss_decode={losses}")
    need(m.get("test_cfg", {}).get("mode", "whole") == "whole", f"model.test_cfg.mode={m.get('test_cfg', {}).get('mode')}")
    for part in ("train", "val"):
        d = cfg["data"][part]
        need(d.get("type") == "NYUDataset", f"data.{part}.type={d.get('type')}")
        need(not d.get("garg_crop", False), f"data.{part}.garg_crop=True")
        need(d.get("split"), f"data.{part}.split={d.get('split')}")
    opt = cfg["optimizer"]
    need(opt.get("type") == "AdamW", f"optimizer.type={opt.get('type')}")
    lr = cfg["lr_config"]
    need(lr.get("policy") == "CosineAnnealing", f"lr_config.policy={lr.get('policy')}")
    need(lr.get("warmup") in ("linear", None), f"lr_config.warmup={lr.get('warmup')}")
    need(not lr.get("by_epoch", False), "lr_config.by_epoch=True")
    mom = cfg.get("momentum_config")
    need(mom is None or mom.get("policy") == "OneCycle", f"momentum_config.policy={(mom or {}).get('policy')}")
    clip = (cfg.get("optimizer_config") or {}).get("grad_clip")
    need(clip is None or clip.get("norm_type", 2) == 2, f"optimizer_config.grad_clip.norm_type={(clip or {}).get('norm_type')}")
    need(cfg["runner"].get("type", "IterBasedRunner") == "IterBasedRunner", f"runner.type={cfg['runner'].get('type')}")
    ev = cfg.get("evaluation", {})
    need(ev.get("save_best", "abs_rel") in DP.METRICS + (None,), f"evaluation.save_best={ev.get('save_best')}")


def build_depth_config(config: str, cfg_options=None, data_root: str | None = None) -> dict:
    cfg = copy.deepcopy(DEPTH_PRESETS[config]) if config in DEPTH_PRESETS else from_file_depth(config)
    apply_cfg_options(cfg, cfg_options)
    if data_root:
        for part in ("train", "val"):
            cfg["data"][part]["data_root"] = data_root
    validate_depth(cfg)
    return cfg


def parse_value(s: str):
    """mmcv DictAction: ints, floats, booleans, None, lists / tuples (`[a,b]`, `(a,b)`, `a,b`), else a string."""
    try:
        return ast.literal_eval(s)
    except (ValueError, SyntaxError):
        pass
    if s in ("True", "False", "None"):
        return {"True": True, "False": False, "None": None}[s]
    if "," in s:
        return [parse_value(v) for v in s.split(",")]
    return s


def apply_cfg_options(cfg: dict, options) -> None:
    for opt in options or []:
        if "=" not in opt:
            raise ValueError(f"--cfg-options expects key=value, got {opt!r}")
        key, val = opt.split("=", 1)
        node = cfg
        parts = key.split(".")
        for p in parts[:-1]:
            if not isinstance(node.get(p), dict):  # a None or scalar on the way is replaced, as mmcv's merge does
                node[p] = {}
            node = node[p]
        node[parts[-1]] = parse_value(val)


def validate(cfg: dict) -> None:
    """Refuse what the port does not implement, naming the value."""
    def need(cond, what):
        if not cond:
            raise NotImplementedError(f"not supported by this port: {what}")
    m = cfg["model"]
    head = m.get("decode_head", {})
    need(m.get("type", "EncoderDecoder") == "EncoderDecoder", f"model.type={m.get('type')}")
    need(head.get("type", "BNHead") == "BNHead", f"model.decode_head.type={head.get('type')}")
    need(head.get("input_transform", "resize_concat") == "resize_concat",
         f"model.decode_head.input_transform={head.get('input_transform')}")
    need(len(head.get("in_index", [3])) == 1, f"model.decode_head.in_index={head.get('in_index')} (one layer only)")
    loss = head.get("loss_decode", {})
    need(loss.get("type", "CrossEntropyLoss") == "CrossEntropyLoss" and not loss.get("use_sigmoid", False)
         and loss.get("loss_weight", 1.0) == 1.0 and not loss.get("avg_non_ignore", False),
         f"model.decode_head.loss_decode={loss}")
    need(not head.get("align_corners", False), "model.decode_head.align_corners=True")
    need(not head.get("dropout_ratio", 0), f"model.decode_head.dropout_ratio={head.get('dropout_ratio')}")
    need(not head.get("resize_factors"), "model.decode_head.resize_factors")
    test = m.get("test_cfg", {})
    need(test.get("mode", "slide") == "slide", f"model.test_cfg.mode={test.get('mode')}")
    for part in ("train", "val"):
        t = cfg["data"][part].get("type")
        need(t in D.DATASETS, f"data.{part}.type={t}")
    opt = cfg["optimizer"]
    need(opt.get("type") == "AdamW", f"optimizer.type={opt.get('type')}")
    lr = cfg["lr_config"]
    need(lr.get("policy") == "poly", f"lr_config.policy={lr.get('policy')}")
    need(lr.get("warmup") in ("linear", None), f"lr_config.warmup={lr.get('warmup')}")
    need(not lr.get("by_epoch", False), "lr_config.by_epoch=True")
    need(cfg["runner"].get("type", "IterBasedRunner") == "IterBasedRunner", f"runner.type={cfg['runner'].get('type')}")
    K = head.get("num_classes", 21)
    need(1 <= K <= 255, f"model.decode_head.num_classes={K}")


def build_config(config: str, cfg_options=None, data_root: str | None = None) -> dict:
    cfg = copy.deepcopy(PRESETS[config]) if config in PRESETS else from_file(config)
    apply_cfg_options(cfg, cfg_options)
    if data_root:
        for part in ("train", "val"):
            cfg["data"][part]["data_root"] = data_root
    validate(cfg)
    return cfg


def get_args(argv=None):
    p = argparse.ArgumentParser("Linear Evaluation (HIP)")
    p.add_argument("config", help="preset (voc2012_linear, ade20k_linear; nyu_linear with --task depth) or a reference-style "
                                  "config file")
    p.add_argument("--work-dir")
    p.add_argument("--load-denoiser-from")
    p.add_argument("--load-distilled-model-from")
    p.add_argument("--num_blocks", type=int, default=1)
    p.add_argument("--resume-from")
    p.add_argument("--backbone-type", default="vit_small_patch14_dinov2.lvd142m")
    p.add_argument("--task", default="segmentation", choices=["segmentation", "depth"])
    p.add_argument("--no-validate", action="store_true")
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--diff_seed", action="store_true")
    p.add_argument("--deterministic", action="store_true")
    p.add_argument("--options", nargs="+", help="deprecated alias of --cfg-options")
    p.add_argument("--cfg-options", nargs="+")
    p.add_argument("--launcher", choices=["none", "pytorch", "slurm", "mpi"], default="pytorch")
    p.add_argument("--local-rank", "--local_rank", type=int, default=0)
    p.add_argument("--auto-resume", action="store_true")
    # this project's
    p.add_argument("--vit_checkpoint", help="timm-layout DINOv2 weights (timm cannot download here)")
    p.add_argument("--allow_random_vit", action="store_true", help="random ViT weights: tests and benchmarks only")
    p.add_argument("--dtype", default="bfloat16", choices=["float32", "bfloat16"], help="extractor arithmetic")
    p.add_argument("--denoiser_dtype", default="float32", choices=["float32", "bfloat16"],
                   help="arithmetic of the --load-denoiser-from denoiser's forward: float32 (exact, the default) or bfloat16 "
                        "(the bf16 extractor's block kernels; needs --dtype bfloat16)")
    p.add_argument("--data-root", help="overrides data.train / data.val data_root")
    a = p.parse_args(argv)
    if a.denoiser_dtype == "bfloat16" and a.dtype == "float32":
        p.error("--denoiser_dtype bfloat16 with --dtype float32 is refused: a bf16 denoiser over an exact-fp32 extractor is "
                "not a mode of the reference; pass --dtype bfloat16 or --denoiser_dtype float32 (nothing was written)")
    kind = config_kind(a.config)
    if kind != a.task:
        p.error(f"{a.config} is a {kind} config, not a {a.task} one: pass --task {kind}")
    if a.launcher in ("slurm", "mpi"):
        p.error(f"--launcher {a.launcher} is not supported: use --launcher pytorch (torchrun) or none")
    return a


# ================================================================================================ models
def build_backbone(args, device):
    """-> (features fn, channels).  Distilled ViT, plain ViT, or the stage-2 Denoiser over the ViT's features."""
    from .models.online_denoiser import Denoiser
    from .models.vit_wrapper import PretrainedViTWrapper
    ckpt = args.load_distilled_model_from or args.vit_checkpoint
    vit = PretrainedViTWrapper(args.backbone_type, stride=int(args.backbone_type.split("patch")[1][:2]),
                               checkpoint_path=ckpt, allow_random_init=args.allow_random_vit and ckpt is None,
                               dtype=args.dtype)
    C = vit.n_output_dims
    den = None
    if args.load_denoiser_from:
        den = Denoiser(noise_map_height=37, noise_map_width=37, feat_dim=C, vit=None, num_blocks=args.num_blocks,
                       device=device, inference_dtype=args.denoiser_dtype)
        sd = torch.load(args.load_denoiser_from, map_location="cpu", weights_only=False)
        den.load_state_dict(sd.get("denoiser", sd), strict=False)
    return S.ViTBackbone(vit._state_dict, vit.patch_size, device, dtype=args.dtype, denoiser=den), C


SEG_TENSORS = ["conv_seg.weight", "conv_seg.bias", "bn.weight", "bn.bias"]  # mmseg's parameter order
DEPTH_TENSORS = ["conv_depth.weight", "conv_depth.bias"]


def optimizer_state(head: S.SegHeadEngine, opt_cfg: dict, lr: float) -> dict:
    """torch.optim.AdamW's state_dict layout over the head's four tensors (mmseg's parameter order)."""
    group = arena.adamw_group(lr, opt_cfg.get("weight_decay", 1e-4), opt_cfg.get("betas", (0.9, 0.999)),
                              initial_lr=opt_cfg["lr"])
    return arena.adamw_state_dict(head, SEG_TENSORS, group, empty_before_first_step=True)


def load_optimizer_state(head: S.SegHeadEngine, st: dict) -> None:
    arena.load_adamw_state(head, SEG_TENSORS, st)


def save_checkpoint(work_dir, head, cfg, it, seed, lr) -> str:
    path = os.path.join(work_dir, f"iter_{it}.pth")
    torch.save({"meta": {"iter": it, "epoch": 0, "seed": seed, "time": time.asctime(),
                         "CLASSES": None, "config": json.dumps(cfg, default=str)},
                "state_dict": head.state_dict(), "optimizer": optimizer_state(head, cfg["optimizer"], lr)}, path)
    shutil.copyfile(path, os.path.join(work_dir, "latest.pth"))
    return path


# ================================================================================================ evaluation
def evaluate(head, backbone, ds, cfg, rank, world, device):
    K = head.K
    hist = torch.zeros(3, K, dtype=torch.int64, device=device)
    test = cfg["model"]["test_cfg"]
    crop, stride = tuple(test.get("crop_size", (512, 512))), tuple(test.get("stride", (341, 341)))
    for i in range(rank, len(ds), world):
        img, lab = D.load_pair(ds, i)
        x = torch.from_numpy(D.test_sample(img, cfg["img_scale"])).to(device)
        lab_t = torch.from_numpy(np.ascontiguousarray(lab)).to(device)
        head.evaluate_image(x, lab_t, hist, backbone, reduce_zero_label=False, crop=crop, stride=stride)
    if world > 1:
        torch.distributed.all_reduce(hist, op=torch.distributed.ReduceOp.SUM)
    return hist.cpu().numpy()


def metrics_table(met: dict, classes) -> str:
    rows = ["+" + "-" * 22 + "+-------+-------+", f"| {'Class':<20} |  IoU  |  Acc  |", "+" + "-" * 22 + "+-------+-------+"]
    for c, iou, acc in zip(classes, met["IoU"], met["Acc"]):
        rows.append(f"| {c:<20} | {100 * iou:5.2f} | {100 * acc:5.2f} |")
    rows.append("+" + "-" * 22 + "+-------+-------+")
    rows.append("Summary:")
    rows.append(f"| aAcc {100 * met['aAcc']:.2f} | mIoU {100 * met['mIoU']:.2f} | mAcc {100 * met['mAcc']:.2f} |")
    return "\n".join(rows)


# ================================================================================================ training
def main(argv=None) -> dict:
    args = get_args(argv)
    # the probe heads' kernels have only been built and measured for the S / B / L widths: a wider backbone stops here, by name
    from .vit import require_consumer_width, require_dinov2_layout
    require_consumer_width(args.backbone_type, "linear-probe evaluation")
    # ... and their data path pads to multiples of 14, normalises with ImageNet's statistics and sizes the denoiser for 37 x 37
    require_dinov2_layout(args.backbone_type, "linear-probe evaluation",
                          "its data path pads to the patch-14 grid and normalises with ImageNet's statistics")
    if args.task == "depth":
        return main_depth(args)
    opts = (args.cfg_options or []) + (args.options or [])
    cfg = build_config(args.config, opts, args.data_root)
    work_dir = args.work_dir or cfg.get("work_dir") or os.path.join(
        "work_dirs", os.path.splitext(os.path.basename(args.config))[0])
    world = int(os.environ.get("WORLD_SIZE", 1)) if args.launcher == "pytorch" else 1
    rank = int(os.environ.get("RANK", 0)) if world > 1 else 0
    local = int(os.environ.get("LOCAL_RANK", args.local_rank)) if world > 1 else 0
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    if world > 1:
        from . import dist as _dist
        _dist.init(device, world)
    os.makedirs(work_dir, exist_ok=True)
    log_path = os.path.join(work_dir, time.strftime("%Y%m%d_%H%M%S") + ".log")

    def log(msg):
        if rank == 0:
            print(msg, flush=True)
            with open(log_path, "a") as f:
                f.write(msg + "\n")

    seed = args.seed if args.seed is not None else 0
    if args.diff_seed:
        seed += rank
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    log(f"Config:\n{json.dumps(cfg, indent=1, default=str)}\nArguments: {json.dumps(vars(args))}\nseed {seed}, world {world}")

    data = cfg["data"]
    tr, va = data["train"], data["val"]
    train_ds = D.DATASETS[tr["type"]](tr["data_root"], "train", tr.get("img_dir"), tr.get("ann_dir"), tr.get("split"))
    val_ds = D.DATASETS[va["type"]](va["data_root"], "val", va.get("img_dir"), va.get("ann_dir"), va.get("split"))
    backbone, C = build_backbone(args, device)
    K = cfg["model"]["decode_head"].get("num_classes", 21)
    head = S.SegHeadEngine(C, K, device, seed=seed)
    classes = train_ds.CLASSES if len(train_ds.CLASSES) == K else tuple(str(i) for i in range(K))

    start = 0
    resume = args.resume_from
    if resume is None and args.auto_resume and os.path.exists(os.path.join(work_dir, "latest.pth")):
        resume = os.path.join(work_dir, "latest.pth")
    if resume:
        ck = torch.load(resume, map_location="cpu", weights_only=False)
        head.load_state_dict(ck["state_dict"])
        load_optimizer_state(head, ck["optimizer"])
        start = int(ck["meta"]["iter"])
        log(f"resumed from {resume} at iter {start}")

    opt, lrc = cfg["optimizer"], cfg["lr_config"]
    T = int(cfg["runner"]["max_iters"])
    spg = int(data["samples_per_gpu"])
    ck_int, ev_int = int(cfg["checkpoint_config"]["interval"]), int(cfg["evaluation"]["interval"])
    log_int = int(cfg.get("log_config", {}).get("interval", 50))
    feeder = D.TrainFeeder(train_ds, spg, cfg["crop_size"], seed, rank, world, start, T, device,
                           workers=min(16, max(1, int(data.get("workers_per_gpu", 4)) * 2)), img_scale=cfg["img_scale"])
    results_path = os.path.join(work_dir, "eval_results.json")
    results = json.load(open(results_path)) if (resume and os.path.exists(results_path)) else []
    lr = 0.0
    t0 = time.perf_counter()
    try:
        for it in range(start, T):
            lr = S.poly_lr(it, opt["lr"], T, lrc.get("power", 1.0), lrc.get("min_lr", 0.0),
                           lrc.get("warmup_iters", 0) if lrc.get("warmup") else 0, lrc.get("warmup_ratio", 0.1))
            img, lab, _ = feeder.next()
            feats = backbone(img)
            stats = None
            if world > 1:
                rec = head.batch_stats(feats)
                gathered = [torch.empty_like(rec) for _ in range(world)]
                torch.distributed.all_gather(gathered, rec)
                stats = head.merge_stats(torch.stack(gathered))
            out = head.train_step(feats, lab, stats=stats)
            if world > 1:
                torch.distributed.all_reduce(head.grads)
            head.adamw_step(lr, opt.get("weight_decay", 1e-4), tuple(opt.get("betas", (0.9, 0.999))),
                            grad_scale=1.0 / world)
            n = it + 1
            if n % log_int == 0 or n == T:
                loss, acc = out.tolist()
                log(f"Iter [{n}/{T}]\tlr: {lr:.3e}, decode.loss_ce: {loss:.4f}, decode.acc_seg: {acc:.4f}, "
                    f"time: {(time.perf_counter() - t0) / max(1, n - start):.3f}")
            if n % ck_int == 0 or n == T:
                if rank == 0:
                    save_checkpoint(work_dir, head, cfg, n, seed, lr)
            if not args.no_validate and (n % ev_int == 0 or n == T):
                hist = evaluate(head, backbone, val_ds, cfg, rank, world, device)
                met = S.total_area_to_metrics(hist)
                log(f"per class results:\n{metrics_table(met, classes)}")
                entry = {"iter": n, "aAcc": met["aAcc"], "mIoU": met["mIoU"], "mAcc": met["mAcc"]}
                for c, iou, acc in zip(classes, met["IoU"], met["Acc"]):
                    entry[f"IoU.{c}"] = None if np.isnan(iou) else float(iou)
                    entry[f"Acc.{c}"] = None if np.isnan(acc) else float(acc)
                results.append(entry)
                if rank == 0:
                    with open(results_path, "w") as f:
                        json.dump(results, f, indent=1)
    finally:
        feeder.close()
    return {"work_dir": work_dir, "results": results}


# ================================================================================================ depth
def depth_optimizer_state(head, opt_cfg: dict, lr: float, beta1: float) -> dict:
    """torch.optim.AdamW's state_dict layout over conv_depth.weight and conv_depth.bias."""
    group = arena.adamw_group(lr, opt_cfg.get("weight_decay", 0.01), (beta1, opt_cfg.get("betas", (0.9, 0.999))[1]),
                              initial_lr=opt_cfg["lr"])
    return arena.adamw_state_dict(head, DEPTH_TENSORS, group, empty_before_first_step=True)


def load_depth_optimizer_state(head, st: dict) -> None:
    arena.load_adamw_state(head, DEPTH_TENSORS, st)


def gather_metric_rows(rows: torch.Tensor, n_total: int, rank: int, world: int) -> torch.Tensor:
    """Rank r holds the rows of images r, r + world, ...: -> the [n_total, 9] table in image order on every rank."""
    if world == 1:
        return rows
    per = -(-n_total // world)
    pad = torch.full((per, rows.shape[1]), float("nan"), dtype=rows.dtype, device=rows.device)
    pad[:rows.shape[0]] = rows
    parts = [torch.empty_like(pad) for _ in range(world)]
    torch.distributed.all_gather(parts, pad)
    return torch.stack([parts[i % world][i // world] for i in range(n_total)])


def evaluate_depth(head, backbone, ds, cfg, rank, world, device) -> np.ndarray:
    """The per-image metric table [n, 9] (float64) of the validation split."""
    crop = DP.EIGEN_CROP if cfg["data"]["val"].get("eigen_crop", True) else None
    mine = list(range(rank, len(ds), world))
    table = torch.zeros(max(len(mine), 1), len(DP.METRICS), dtype=torch.float64, device=device)
    for j, i in enumerate(mine):
        img, depth = DD.load_pair(ds, i)
        x = torch.from_numpy(DD.test_sample(img)).to(device)
        gt = torch.from_numpy(np.ascontiguousarray(depth)).to(device)
        head.evaluate_image(x, gt, table[j], backbone, crop=crop)
    return gather_metric_rows(table[:len(mine)], len(ds), rank, world).cpu().numpy()


def main_depth(args) -> dict:
    opts = (args.cfg_options or []) + (args.options or [])
    cfg = build_depth_config(args.config, opts, args.data_root)
    work_dir = args.work_dir or cfg.get("work_dir") or os.path.join(
        "work_dirs", os.path.splitext(os.path.basename(args.config))[0])
    world = int(os.environ.get("WORLD_SIZE", 1)) if args.launcher == "pytorch" else 1
    rank = int(os.environ.get("RANK", 0)) if world > 1 else 0
    local = int(os.environ.get("LOCAL_RANK", args.local_rank)) if world > 1 else 0
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    if world > 1:
        from . import dist as _dist
        _dist.init(device, world)
    os.makedirs(work_dir, exist_ok=True)
    log_path = os.path.join(work_dir, time.strftime("%Y%m%d_%H%M%S") + ".log")

    def log(msg):
        if rank == 0:
            print(msg, flush=True)
            with open(log_path, "a") as f:
                f.write(msg + "\n")

    seed = args.seed if args.seed is not None else 0
    if args.diff_seed:
        seed += rank
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    log(f"Config:\n{json.dumps(cfg, indent=1, default=str)}\nArguments: {json.dumps(vars(args))}\nseed {seed}, world {world}")

    data = cfg["data"]
    tr, va = data["train"], data["val"]
    train_ds = DD.NYUDataset(tr["data_root"], tr["split"], tr.get("depth_scale", 1000))
    val_ds = DD.NYUDataset(va["data_root"], va["split"], va.get("depth_scale", 1000))
    backbone, C = build_backbone(args, device)
    backbone.return_cls = True
    hc = cfg["model"]["decode_head"]
    head = DP.DepthHeadEngine(C, device, n_bins=hc.get("n_bins", 256), min_depth=hc.get("min_depth", 1e-3),
                              max_depth=hc.get("max_depth", 10), upsample=hc.get("upsample", 4), seed=seed)

    start, best = 0, None
    resume = args.resume_from
    if resume is None and args.auto_resume and os.path.exists(os.path.join(work_dir, "latest.pth")):
        resume = os.path.join(work_dir, "latest.pth")
    if resume:
        ck = torch.load(resume, map_location="cpu", weights_only=False)
        head.load_state_dict(ck["state_dict"])
        load_depth_optimizer_state(head, ck["optimizer"])
        start = int(ck["meta"]["iter"])
        best = ck["meta"].get("best")
        log(f"resumed from {resume} at iter {start}")

    opt, lrc = cfg["optimizer"], cfg["lr_config"]
    T = int(cfg["runner"]["max_iters"])
    spg = int(data["samples_per_gpu"])
    ckc, evc = cfg["checkpoint_config"], cfg["evaluation"]
    ck_int, ev_int, keep = int(ckc["interval"]), int(evc["interval"]), int(ckc.get("max_keep_ckpts", -1))
    log_int = int(cfg.get("log_config", {}).get("interval", 50))
    clip = (cfg.get("optimizer_config") or {}).get("grad_clip")
    onecycle = cfg.get("momentum_config") is not None
    betas = tuple(opt.get("betas", (0.9, 0.999)))
    key, rule = evc.get("save_best", "abs_rel"), evc.get("rule") or ("greater" if evc.get("save_best") in ("a1", "a2", "a3") else "less")
    feeder = DD.DepthTrainFeeder(train_ds, spg, cfg["crop_size"], seed, rank, world, start, T, device,
                                 workers=min(16, max(1, int(data.get("workers_per_gpu", 2)) * 2)))
    results_path = os.path.join(work_dir, "eval_results.json")
    results = json.load(open(results_path)) if (resume and os.path.exists(results_path)) else []
    results = [r for r in results if r["iter"] <= start]
    lr, beta1, skipped = 0.0, betas[0], 0
    t0 = time.perf_counter()

    def save(name, n):
        path = os.path.join(work_dir, name)
        torch.save({"meta": {"iter": n, "epoch": 0, "seed": seed, "time": time.asctime(), "best": best,
                             "config": json.dumps(cfg, default=str)},
                    "state_dict": head.state_dict(), "optimizer": depth_optimizer_state(head, opt, lr, beta1)}, path)
        return path

    try:
        for it in range(start, T):
            lr = DP.cosine_lr(it, opt["lr"], T, lrc.get("min_lr_ratio", 0.0), lrc.get("warmup_iters", 0) if lrc.get("warmup") else 0,
                              lrc.get("warmup_ratio", 0.1))
            beta1 = DP.onecycle_beta1(it, T) if onecycle else betas[0]
            img, gt, _, valid = feeder.next()
            n = it + 1
            if world == 1 and not valid:
                # the reference's loss is NaN here and poisons the head: the step is skipped, the parameters stay as they are
                skipped += 1
                log(f"Iter [{n}/{T}]\tskipped: no valid ground-truth pixel in the batch ({skipped} so far)")
                out = None
            else:
                feats, cls = backbone(img)
                out = head.train_step(feats, cls, gt, it)
                if world > 1:  # a rank without a valid pixel joins with zero gradients; the loss statistics stay per rank
                    torch.distributed.all_reduce(head.grads)
                    head.grads.mul_(1.0 / world)
                if clip:
                    head.clip_grad_norm(float(clip["max_norm"]))
                head.adamw_step(lr, opt.get("weight_decay", 0.01), (beta1, betas[1]))
            if out is not None and (n % log_int == 0 or n == T):
                ld, lg = out.tolist()
                log(f"Iter [{n}/{T}]\tlr: {lr:.3e}, momentum: {beta1:.4f}, decode.loss_depth: {ld:.4f}, decode.loss_grad: {lg:.4f}, "
                    f"loss: {ld + lg:.4f}, time: {(time.perf_counter() - t0) / max(1, n - start):.3f}")
            if (n % ck_int == 0 or n == T) and rank == 0:
                path = save(f"iter_{n}.pth", n)
                shutil.copyfile(path, os.path.join(work_dir, "latest.pth"))
                if keep > 0:
                    old = sorted((int(f[5:-4]) for f in os.listdir(work_dir) if f.startswith("iter_") and f.endswith(".pth")))
                    for m_ in old[:-keep]:
                        os.remove(os.path.join(work_dir, f"iter_{m_}.pth"))
            if not args.no_validate and (n % ev_int == 0 or n == T):
                table = evaluate_depth(head, backbone, val_ds, cfg, rank, world, device)
                met = DP.summarize(table)
                log("Summary:\n" + " | ".join(f"{k} {v:.4f}" for k, v in met.items()))
                results.append({"iter": n, **met})
                if rank == 0:
                    with open(results_path, "w") as f:
                        json.dump(results, f, indent=1)
                    v = met.get(key) if key else None
                    if v is not None and not np.isnan(v) and (best is None or (v < best["value"] if rule == "less" else v > best["value"])):
                        if best is not None and os.path.exists(os.path.join(work_dir, best["file"])):
                            os.remove(os.path.join(work_dir, best["file"]))
                        best = {"value": v, "iter": n, "file": f"best_{key}_iter_{n}.pth"}
                        save(best["file"], n)
    finally:
        feeder.close()
    return {"work_dir": work_dir, "results": results, "skipped": skipped}


if __name__ == "__main__":
    main()
