"""Stage-3 driver: distil the stage-2 denoiser's output into the ViT itself (the `*_distilled` checkpoints).

Mirrors the reference's main_distillation.py (flags :26-84, setup :106-213, loop :218-296): the student is the whole
ViT, trained in fp32 on `get_intermediate_layers(n=1, norm=True)` features; the teacher is `Denoiser(vit=...)` loaded from
the stage-2 checkpoint, run under no_grad; loss = MSE + (1 - cosine) over the patch tokens; AdamW over every tensor in one
param group (weight decay on all of them); sqrt-scaled learning rate with a cosine schedule and 15 % warm-up from 0;
rank-0 checkpoints `{model, optimizer, step}` with `model.`-prefixed timm keys + a `latest.pth` symlink.

Any `--input_size` / `--stride_size`: when the run's token grid is not the grid of the checkpoint's position table, the
student keeps `pos_embed` at the CHECKPOINT's shape (parameters, gradients, both AdamW moments, the written checkpoints) and
every step resamples it to the run's grid and carries the gradient back through the transpose of that map
(dvt_pos_resample_fwd / _bwd in csrc/dvt_stage3.hip) -- timm's dynamic_img_size forward and its autograd.

MI355X layout: one process per GPU (`python -m torch.distributed.run --nproc-per-node N -m dvt_amd.stage3 ...`).  Every
rank runs the teacher (csrc/dvt_vit_f32.hip + csrc/dvt_stage2.hip) and the student's forward + loss + backward
(csrc/dvt_stage3.hip) on its own batch; the student's gradients are ONE flat fp32 arena, summed across ranks by one
all-reduce per step and scaled by 1/world inside the AdamW kernel (the reference wraps the student in DDP).

Deviations, all forced or harmless:
  * `--input_size` takes two values (what stage3.sh passes) or none (518 x 518).  One value is refused: the reference then
    resizes the short side, and images of different aspect ratios cannot be batched.
  * the teacher is built at the grid of the denoiser checkpoint's `pos_embed` (its square row count) and serves the run's
    grid from a resampled inference copy (`Denoiser._engine_for`): the reference's `Denoiser.forward` resamples its table to
    the input's grid too, only its `load_state_dict` ties the constructor's grid to the checkpoint.  A checkpoint without
    `pos_embed` (a denoiser trained with enable_pe=False) runs at any grid, without one.
  * the horizontal flip is drawn from numpy's default_rng((seed, step, position in the global batch)), not from the
    DataLoader workers' torch RNG, which cannot be reproduced outside torch's worker processes.
  * `--grad_checkpointing` recomputes nothing: a batch that does not fit is split into slices (`--micro_batch`) whose
    gradients add up to the whole batch's.
  * PCA visualisations are not written (`--vis_freq` / `--num_vis_samples` are accepted).
  * `--dtype bfloat16` (default float32, what the reference trains in) is an opt-in mixed-precision student step: see
    dvt_amd/s3.py and include/dvt_stage3.h.  Parameters, optimizer state and checkpoints are fp32 either way, so a
    checkpoint written under one dtype starts a run under the other through `--vit_checkpoint`.  `--attention bfloat16`
    (default float32) adds the bf16 flash attention on top of `--dtype bfloat16` and is refused without it; so is
    `--weight_grad bfloat16` (default float32), which forms the blocks' weight gradients from bf16 operands.
  * the ViT weights come from `--vit_checkpoint` (a timm-layout state dict, or a stage-3 checkpoint) because timm cannot
    download here; `--allow_random_vit` runs on random weights (tests and plumbing only).
"""
from __future__ import annotations

import argparse
import math
import os
import queue
import re
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.distributed as dist

from . import arena
from . import dist as D
from .models.vit_wrapper import IMAGENET_MEAN, IMAGENET_STD, MODEL_LIST
from .stage2 import CosineScheduler, sampler_indices
from .utils import misc
from . import _lib
from .vit import SPECS, model_statistics, require_dinov2_layout

# torchvision.datasets.folder.IMG_EXTENSIONS
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")


# ---- data ----------------------------------------------------------------------------------------------------
class ImageFolderList:
    """torchvision `ImageFolder(root)` restated (absent here): classes = sorted sub-directories, samples = for each class a
    sorted recursive walk (links followed), files sorted, kept when the lower-cased name ends with IMG_EXTENSIONS."""

    def __init__(self, root: str):
        self.root = root
        self.classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
        if not self.classes:
            raise FileNotFoundError(f"no class folders under {root}")
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        self.samples = []
        for c in self.classes:
            for dirpath, _, fnames in sorted(os.walk(os.path.join(root, c), followlinks=True)):
                for f in sorted(fnames):
                    if f.lower().endswith(IMG_EXTENSIONS):
                        self.samples.append((os.path.join(dirpath, f), self.class_to_idx[c]))
        if not self.samples:
            raise FileNotFoundError(f"no images with extensions {IMG_EXTENSIONS} under {root}")

    def __len__(self):
        return len(self.samples)


def flip_decision(seed: int, step: int, position: int) -> bool:
    """RandomHorizontalFlip's coin for the image at `position` of the global batch of `step`."""
    return bool(np.random.default_rng((seed, step, position)).random() < 0.5)


def load_image(path: str, size: tuple, flip: bool, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> np.ndarray:
    """main_distillation.py's transform: PIL decode -> RGB -> Resize(size, BICUBIC, antialias) -> flip -> ToTensor ->
    Normalize with the model's statistics (`model_statistics`); -> fp32 [3, H, W]."""
    from PIL import Image
    with open(path, "rb") as f:
        img = Image.open(f).convert("RGB")
    h, w = size
    img = img.resize((w, h), Image.BICUBIC)
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    a = np.asarray(img, dtype=np.float32) / 255.0
    a = (a - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    return np.ascontiguousarray(a.transpose(2, 0, 1))


class ImageFeeder:
    """Decodes `batch_size` images per step in a host thread pool into one of `depth` pinned buffers and uploads them on a
    side stream, as stage 2's BatchFeeder does; `next()` hands out a device tensor [B, 3, H, W] whose copy the compute
    stream waits for."""

    def __init__(self, ds: ImageFolderList, indices, batch_size, size, device, seed, first_step, rank,
                 workers=8, depth=2, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        self.ds, self.it, self.bs, self.size, self.device = ds, indices, batch_size, tuple(size), device
        self.mean, self.std = tuple(mean), tuple(std)
        self.seed, self.step, self.rank = seed, first_step, rank
        self.pool = ThreadPoolExecutor(max(1, workers))
        cuda = device.type == "cuda"
        self.copy_stream = torch.cuda.Stream(device) if cuda else None
        shape = (batch_size, 3, *self.size)
        self.host = [torch.empty(shape, dtype=torch.float32, pin_memory=cuda) for _ in range(depth)]
        self.dev = [torch.empty(shape, dtype=torch.float32, device=device) for _ in range(depth)]
        self.events = [None] * depth
        self.free, self.ready = queue.Queue(), queue.Queue(maxsize=depth)
        for i in range(depth):
            self.free.put(i)
        self.stop = False
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def _load_one(self, slot, step, j, index):
        flip = flip_decision(self.seed, step, self.rank * self.bs + j)
        self.host[slot][j].copy_(torch.from_numpy(load_image(self.ds.samples[index][0], self.size, flip, self.mean, self.std)))

    def _run(self):
        try:
            while not self.stop:
                slot = self.free.get()
                if slot is None:
                    return
                step = self.step
                self.step += 1
                idx = [next(self.it) for _ in range(self.bs)]
                list(self.pool.map(lambda a: self._load_one(slot, step, *a), enumerate(idx)))
                if self.copy_stream is not None:
                    with torch.cuda.stream(self.copy_stream):
                        self.dev[slot].copy_(self.host[slot], non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record(self.copy_stream)
                    self.events[slot] = ev
                else:
                    self.dev[slot].copy_(self.host[slot])
                self.ready.put(slot)
        except BaseException as e:  # surface reader failures in the training thread
            self.ready.put(e)

    def next(self):
        slot = self.ready.get()
        if isinstance(slot, BaseException):
            raise slot
        if self.events[slot] is not None:
            torch.cuda.current_stream(self.device).wait_event(self.events[slot])
        return slot, self.dev[slot]

    def release(self, slot, done_event=None):
        if done_event is not None:
            done_event.synchronize()
        self.free.put(slot)

    def close(self):
        self.stop = True
        self.free.put(None)
        self.pool.shutdown(wait=False)


# ---- checkpoints ---------------------------------------------------------------------------------------------
def timm_order(names) -> list:
    """`VisionTransformer.named_parameters()` order: its own parameters (cls_token, reg_token, pos_embed), then
    patch_embed, blocks, norm."""
    head = [n for n in ("cls_token", "reg_token", "pos_embed") if n in names]
    rest = [n for n in names if n not in head]
    return head + rest


def optimizer_state(eng, lr: float, weight_decay: float) -> dict:
    """`torch.optim.AdamW.state_dict()` of the student's parameters, built from the flat moments."""
    return arena.adamw_state_dict(eng, timm_order(list(eng.views())),
                                  arena.adamw_group(lr, weight_decay, **arena.TORCH2_GROUP_DEFAULTS))


def model_state(eng) -> dict:
    """The wrapper's state_dict: `model.<timm key>` (PretrainedViTWrapper holds the timm model as `.model`)."""
    sd = eng.state_dict()
    return {"model." + k: sd[k] for k in timm_order(list(sd))}


def save_checkpoint(log_dir: str, eng, step: int, lr: float, weight_decay: float) -> str:
    """main_distillation.py:264-282: ckpt_{step:06d}.pth + latest.pth symlink."""
    path = f"{log_dir}/checkpoints/ckpt_{step:06d}.pth"
    torch.save({"model": model_state(eng), "optimizer": optimizer_state(eng, lr, weight_decay), "step": step}, path)
    arena.link_latest(path, f"{log_dir}/checkpoints/latest.pth")
    return path


# ---- CLI -----------------------------------------------------------------------------------------------------
def get_args(argv=None):
    p = argparse.ArgumentParser("Distil the denoiser into the ViT (MI355X)")
    p.add_argument("--model", type=str, default="vit_base_patch14_dinov2.lvd142m", choices=MODEL_LIST)
    p.add_argument("--num_blocks", type=int, default=1)
    p.add_argument("--denoiser_ckpt", type=str, required=True)
    p.add_argument("--grad_checkpointing", action="store_true",
                   help="accepted; nothing is recomputed here -- use --micro_batch to bound the activation memory")
    p.add_argument("--data_root", type=str, default="data/imagenet")
    p.add_argument("--feat_root", type=str, default=None)
    p.add_argument("--data_list_path", type=str, default=None)
    p.add_argument("--input_size", type=int, default=518, nargs="+")
    p.add_argument("--auto_stride", action="store_true", help="set stride size = patch size.")
    p.add_argument("--stride_size", type=int, default=14, help="Stride size for the model.")
    p.add_argument("--num_workers", default=8, type=int)
    p.add_argument("--batch_size", default=32, type=int, help="Batch size per GPU")
    p.add_argument("--num_vis_samples", default=8, type=int)
    p.add_argument("--num_iterations", default=None, type=int)
    p.add_argument("--num_epochs", default=10, type=int)
    p.add_argument("--weight_decay", type=float, default=1e-5)
    p.add_argument("--blr", type=float, default=2.0e-04, help="abs_lr = blr * sqrt(total_bs / 256)")
    p.add_argument("--min_lr", type=float, default=1.0e-06, help="for cosine scheduler")
    p.add_argument("--warmup_iters", type=int, default=50_000, help="parsed, unused (the warm-up is 15 %% of the run)")
    p.add_argument("--output_root", default="./work_dirs/", type=str)
    p.add_argument("--save_freq", default=5000, type=int)
    p.add_argument("--vis_freq", default=5000, type=int)
    p.add_argument("--project", default="denosing-vit", type=str)
    p.add_argument("--run_name", default="debug", type=str)
    p.add_argument("--seed", default=42, type=int)
    p.add_argument("--world_size", default=1, type=int, help="accepted; the world comes from torch.distributed.run")
    p.add_argument("--local_rank", "--local-rank", default=-1, type=int)
    p.add_argument("--dist_on_itp", action="store_true")
    p.add_argument("--dist_url", default="env://")
    p.add_argument("--distributed", action="store_true")
    p.add_argument("--device", default="cuda", help="device to use for training / testing")
    # not in the reference
    p.add_argument("--vit_checkpoint", type=str, default=None, help="timm-layout state dict (.pth) or a stage-3 checkpoint")
    p.add_argument("--allow_random_vit", action="store_true", help="random ViT weights (tests / plumbing runs only)")
    p.add_argument("--micro_batch", type=int, default=0,
                   help="images per slice of the student's step; 0 = as many as fit in 80 %% of the free device memory")
    p.add_argument("--log_freq", default=50, type=int)
    p.add_argument("--dtype", default="float32", choices=["float32", "bfloat16"],
                   help="float32 (default): the student's step in exact fp32, as the reference trains.  bfloat16: the forward "
                        "and data-gradient GEMMs of the blocks' linear layers take bf16 operands (fp32 accumulation); weight "
                        "gradients, parameters, optimizer state, checkpoints and the teacher stay fp32")
    p.add_argument("--attention", default="float32", choices=["float32", "bfloat16"],
                   help="float32 (default): the student's attention as fp32 products with the probabilities kept.  bfloat16 "
                        "(needs --dtype bfloat16): bf16 flash attention -- q, k, v, P, dS and d ao are rounded to bf16 as "
                        "matrix operands, accumulation in fp32; the backward recomputes the probabilities from a per-row "
                        "log-sum-exp, so no [tokens, tokens] matrix is kept and larger slices fit")
    p.add_argument("--weight_grad", default="float32", choices=["float32", "bfloat16"],
                   help="float32 (default): the blocks' weight gradients in exact fp32.  bfloat16 (needs --dtype bfloat16): "
                        "dW = bf16(dy)^T bf16(x) on the bf16 split-K kernel, fp32 accumulation; bias gradients, the patch "
                        "embedding's gradient, parameters, optimizer state and checkpoints stay fp32")
    p.add_argument("--teacher_dtype", default="float32", choices=["float32", "bfloat16"],
                   help="float32 (default): the teacher -- the ViT extractor and the stage-2 denoiser over it -- in exact fp32.  "
                        "bfloat16: the teacher's forward on the bf16 extractor with the denoiser's block fused behind it (one "
                        "launch sequence from image to denoised features); the student, its weights and every student mode "
                        "do not depend on it")
    args = p.parse_args(argv)
    if args.attention == "bfloat16" and args.dtype != "bfloat16":
        from .s3 import ATTENTION_NEEDS_BF16
        raise SystemExit("stage 3: " + ATTENTION_NEEDS_BF16)
    if args.weight_grad == "bfloat16" and args.dtype != "bfloat16":
        from .s3 import WEIGHT_GRAD_NEEDS_BF16
        raise SystemExit("stage 3: " + WEIGHT_GRAD_NEEDS_BF16)
    if isinstance(args.input_size, int):
        args.input_size = (args.input_size, args.input_size)
    elif len(args.input_size) == 1:
        raise SystemExit("--input_size needs two values (H W), as stage3.sh passes them: with one value the reference "
                         "resizes the short side, and images of different aspect ratios cannot be batched")
    elif len(args.input_size) != 2:
        raise SystemExit("--input_size takes two values (H W)")
    args.input_size = tuple(args.input_size)
    if args.auto_stride:
        args.stride_size = int(re.search(r"patch(\d+)", args.model).group(1))
    if args.stride_size in (8, 16) and args.input_size[0] == 518:
        args.input_size = (512, 512)
    if args.input_size[0] % args.stride_size or args.input_size[1] % args.stride_size:
        raise SystemExit("input size must be divisible by stride_size")
    return args


def geometry(args):
    """(dim, depth, patch, grid_h, grid_w, n_reg) of the student at this input size and stride."""
    if args.model not in SPECS:
        raise NotImplementedError(f"{args.model}: the stage-3 trainer takes the DINOv2 S/B/L (+reg4) ViTs of dvt_amd.vit.SPECS only")
    # the trainer's parameter arena holds LayerScale as trained tensors and derives the position table's cls row from the
    # registers: the DINO / AugReg (no LayerScale) and DeiT-III (no cls row, no registers) layouts stop here, by name
    require_dinov2_layout(args.model, "the stage-3 trainer", "its parameter arena trains ls1 / ls2 and a DINOv2 position table")
    s = SPECS[args.model]
    return (s.dim, s.depth, s.patch, (args.input_size[0] - s.patch) // args.stride_size + 1,
            (args.input_size[1] - s.patch) // args.stride_size + 1, s.n_reg)


def num_iterations(args, n_images: int, world: int) -> int:
    """main_distillation.py:186-189: steps_per_epoch * num_epochs unless --num_iterations is given."""
    if args.num_iterations is not None:
        return args.num_iterations
    return n_images // (args.batch_size * world) * args.num_epochs


def learning_rate(args, world: int) -> float:
    return args.blr * math.sqrt(args.batch_size * world / 256)


def scheduler(args, lr: float, n_iter: int) -> CosineScheduler:
    return CosineScheduler(lr, args.min_lr, n_iter, warmup_iters=int(n_iter * 0.15), start_warmup_value=0)


def square_grid(n_rows: int, what: str) -> int:
    g = math.isqrt(max(int(n_rows), 0))
    if g < 1 or g * g != n_rows:
        raise _lib.DvtError(f"{what} with {n_rows} patch positions is not a square grid")
    return g


def teacher_grid(den_sd: dict, dim: int, gh: int, gw: int) -> tuple:
    """(noise_map_height, noise_map_width) to build the teacher at: the run's grid when the denoiser checkpoint has no
    `pos_embed` or has one of exactly gh * gw rows, else the square grid of its rows (`Denoiser._engine_for` then serves the
    run's grid)."""
    pe = den_sd.get("pos_embed")
    if pe is None or pe.numel() // dim == gh * gw:
        return gh, gw
    g = square_grid(pe.numel() // dim, "the denoiser checkpoint's pos_embed")
    return g, g


def build_models(args, device):
    """-> (student engine, teacher).  The teacher is `Denoiser(vit=PretrainedViTWrapper(..., dtype="float32"))` with the
    stage-2 checkpoint loaded non-strictly (main_distillation.py:131-141); the student starts from the same ViT weights.
    --teacher_dtype bfloat16 builds the wrapper with dtype="bfloat16" and the Denoiser with inference_dtype="bfloat16" (the
    fused bf16 forward); the student is loaded from the wrapper's fp32 `_state_dict` either way."""
    from .models.online_denoiser import Denoiser
    from .models.vit_wrapper import PretrainedViTWrapper
    from .s3 import Stage3Engine, make_config
    dim, depth, patch, gh, gw, n_reg = geometry(args)
    teacher_dtype = getattr(args, "teacher_dtype", "float32")
    if teacher_dtype not in ("float32", "bfloat16"):
        raise ValueError(f"teacher_dtype must be 'float32' or 'bfloat16', not {teacher_dtype!r}")
    bf16_teacher = {"inference_dtype": "bfloat16"} if teacher_dtype == "bfloat16" else {}  # float32: built as it always was
    vit = PretrainedViTWrapper(args.model, stride=args.stride_size, checkpoint_path=args.vit_checkpoint,
                               img_size=args.input_size, allow_random_init=args.allow_random_vit, dtype=teacher_dtype)
    den_sd = torch.load(args.denoiser_ckpt, map_location="cpu", weights_only=False)["denoiser"]
    teacher = Denoiser(*teacher_grid(den_sd, dim, gh, gw), feat_dim=dim, vit=vit, enable_pe="pos_embed" in den_sd,
                       num_blocks=args.num_blocks, device=device, **bf16_teacher)
    teacher.load_state_dict(den_sd, strict=False)
    # the wrapper keeps the checkpoint's table un-resampled: its grid is what the student trains
    g0 = square_grid(vit._state_dict["pos_embed"].shape[-2] - SPECS[args.model].pos_has_cls, "the ViT checkpoint's pos_embed")
    pos_grid = None if (g0, g0) == (gh, gw) else g0
    if pos_grid is not None:
        print(f"stage 3: position table {g0} x {g0} resampled to {gh} x {gw} in every step", flush=True)
    student = Stage3Engine(make_config(dim, depth, patch, args.stride_size, *args.input_size, n_reg), device,
                           pos_grid=pos_grid, dtype=args.dtype, attention=args.attention,
                           weight_grad=getattr(args, "weight_grad", "float32"))
    student.load_timm(vit._state_dict)
    return student, teacher


def train(args, rank: int, world: int, device: torch.device, model_factory=None) -> dict:
    """The loop of main_distillation.py:218-296.  `model_factory(args, device) -> (student engine, teacher)` lets the CPU
    tests inject stand-ins with the engine interface (the product engine needs a HIP device)."""
    distributed = world > 1
    if model_factory is None:
        geometry(args)  # a model the trainer is not built for stops here, before the run directory exists
    mean, std = model_statistics(args.model)
    log_dir = os.path.join(args.output_root, args.project, args.run_name)
    if rank == 0:
        os.makedirs(f"{log_dir}/checkpoints", exist_ok=True)
        if args.grad_checkpointing:
            print("stage 3: --grad_checkpointing recomputes nothing here; --micro_batch bounds the activation memory",
                  flush=True)
        print("stage 3: PCA visualisations are not written (--vis_freq / --num_vis_samples are accepted)", flush=True)
        print(f"stage 3: student step dtype {args.dtype}"
              + (" (bf16 operands in the forward and data-gradient GEMMs of the linear layers; weight gradients, state and "
                 "checkpoints fp32)" if args.dtype == "bfloat16" else " (exact fp32)"), flush=True)
        print(f"stage 3: student attention {args.attention}"
              + (" (bf16 flash attention: fp32 accumulation, probabilities recomputed in the backward pass, none kept)"
                 if args.attention == "bfloat16" else " (fp32 products, probabilities kept)"), flush=True)
        print(f"stage 3: teacher dtype {getattr(args, 'teacher_dtype', 'float32')}"
              + (" (bf16 extractor with the denoiser fused behind it)"
                 if getattr(args, "teacher_dtype", "float32") == "bfloat16" else " (exact fp32 extractor and denoiser)"), flush=True)
        if getattr(args, "weight_grad", "float32") == "bfloat16":
            print("stage 3: student weight gradients bfloat16 (bf16 operands on the split-K kernel, fp32 accumulation; bias "
                  "gradients fp32)", flush=True)
    misc.fix_random_seeds(args.seed)
    eng, teacher = (model_factory or build_models)(args, device)
    if distributed:  # DistributedDataParallel broadcasts rank 0's parameters at construction
        dist.broadcast(eng.params, src=0)
    ds = ImageFolderList(args.data_root)
    n_iter = num_iterations(args, len(ds), world)
    lr_base = learning_rate(args, world)
    sched = scheduler(args, lr_base, n_iter)
    feeder = ImageFeeder(ds, sampler_indices(len(ds), world, rank, distributed), args.batch_size, args.input_size, device,
                         args.seed, 0, rank, workers=args.num_workers, mean=mean, std=std)
    micro = args.micro_batch if args.micro_batch > 0 else None
    history, t_log = [], time.time()
    pending = []
    # sticky non-finite flag, reduced over ranks at log and save steps (as the stage-2 driver): the reference stops on the
    # first non-finite loss; here every rank stops together and no poisoned parameters reach a checkpoint
    bad = torch.zeros((), device=device, dtype=torch.float32)
    bad_step = torch.full((), float("inf"), device=device, dtype=torch.float32)

    def raise_if_bad(step):
        flag = torch.stack([bad, -bad_step])
        if distributed:
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        b, neg_at = flag.cpu().tolist()
        if b != 0.0:
            raise FloatingPointError(f"loss is not finite (first seen at step {int(-neg_at)}, detected at step {step}), "
                                     "stopping training")

    try:
        for step in range(n_iter):
            lr = float(sched[step])
            slot, img = feeder.next()
            with torch.no_grad():
                target = teacher(img, return_dict=True)["denoised_feats"].contiguous()
            loss = eng.train_step(img, target, micro_batch=micro)
            nf = (~torch.isfinite(loss.detach()[0])).float()
            bad_step = torch.where((bad == 0) & (nf != 0), torch.full_like(bad_step, float(step)), bad_step)
            bad = torch.maximum(bad, nf)
            if distributed:
                dist.all_reduce(eng.grads)  # SUM; the mean over ranks is taken inside the AdamW kernel
            eng.adamw_step(lr, args.weight_decay, grad_scale=1.0 / world)
            ev = None
            if device.type == "cuda":
                ev = torch.cuda.Event()
                ev.record()
            pending.append((slot, ev))
            if len(pending) > 1:
                feeder.release(*pending.pop(0))
            is_log = step % args.log_freq == 0 or step == n_iter - 1
            is_save = step % args.save_freq == 0 or step == n_iter - 1
            if is_log or is_save:
                raise_if_bad(step)
            if is_log:
                vals = loss.detach().cpu().tolist()
                now = time.time()
                last = {"step": step, "loss": vals[0], "l2_loss": vals[1], "cosine_similarity_loss": vals[2], "lr": lr,
                        "iter_time": (now - t_log) / max(1, args.log_freq if step else 1)}
                t_log = now
                history.append(last)
                if rank == 0:
                    print("Train  [{step}/{n}]  loss: {loss:.6f}  l2_loss: {l2_loss:.6f}  cosine_similarity_loss: "
                          "{cosine_similarity_loss:.6f}  lr: {lr:.3e}  iter_time: {iter_time:.4f}".format(n=n_iter, **last),
                          flush=True)
            if rank == 0 and is_save:
                save_checkpoint(log_dir, eng, step, lr, args.weight_decay)
    finally:
        feeder.close()
    return {"log_dir": log_dir, "history": history, "engine": eng, "teacher": teacher, "num_iterations": n_iter}


def main(argv=None):
    args = get_args(argv)
    rank, world, local = D.env_ranks()
    device = torch.device(args.device, local) if args.device == "cuda" else torch.device(args.device)
    if device.type == "cuda":
        torch.cuda.set_device(device)
    D.init(device, world)
    try:
        train(args, rank, world, device)
    finally:
        D.finish()


if __name__ == "__main__":
    sys.exit(main())
