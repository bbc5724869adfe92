"""Host side of the linear-probe depth evaluation (csrc/dvt_depth.hip, C ABI in include/dvt_depth.h).

The reference evaluates features with `evaluate_dense_tasks.py --task depth` and `vitb_nyu_linear_config.py`: its depth
`BNHead` (no norm layer: the cls token broadcast behind the patch tokens, a x4 bilinear upsample, `conv_depth` = a 1 x 1
convolution to 256 bins, a linear normalisation and the expectation over uniform bins) trained on frozen backbone features
with SigLoss + GradientLoss, then flip-averaged whole-image inference and the nine NYU metrics.  `DepthHeadEngine` owns that
head: flat fp32 parameter / gradient / AdamW-moment arenas (layout of `dvt_depth_param_offsets`, stepped by `dvt_adamw_step`).

The pure host pieces (the schedules, the metric table's summary, the checkpoint layout) are plain Python, so that they can be
checked without a GPU.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .arena import FlatAdamW

_P, _I, _I64, _F = C.c_void_p, C.c_int, C.c_int64, C.c_float
_lib.register_signatures({
    "dvt_depth_param_offsets": (_I, [_I, _I, C.POINTER(C.c_int64)]),
    "dvt_depth_workspace_bytes": (_I64, [_I, _I, _I, _I, _I, _I, _I, _I]),
    "dvt_depth_forward": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _I64, _P]),
    "dvt_depth_train_step": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _P, _I64, _P, _P]),
    "dvt_depth_clip_work_floats": (_I64, [_I64]),
    "dvt_depth_clip_grad_norm": (_I, [_P, _I64, _F, _P, _P, _P]),
    "dvt_depth_eval_work_bytes": (_I64, [_I, _I]),
    "dvt_depth_eval_image": (_I, [_P, _P, _I, _I, _P, _I, _I, _F, _F, _I, _I, _I, _I, _P, _P, _P, _P]),
})

METRICS = ("a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel")
WARM_ITERS = 100            # SigLoss warm_iter
GRAD_LOSS_WEIGHT = 0.5      # GradientLoss loss_weight of the config
EIGEN_CROP = (45, 471, 41, 601)  # NYU: rows [45, 471), columns [41, 601)


# ================================================================================================ pure host pieces
def cosine_lr(it: int, base_lr: float, max_iters: int, min_lr_ratio: float = 1e-8, warmup_iters: int = 12800,
              warmup_ratio: float = 1e-3) -> float:
    """mmcv 1.x CosineAnnealingLrUpdaterHook (by_epoch=False) under a linear warm-up, at 0-based iteration `it`
    (restated from its published behaviour; the warm-up formula is seg.poly_lr's)."""
    target = base_lr * min_lr_ratio
    lr = target + 0.5 * (base_lr - target) * (math.cos(math.pi * it / max_iters) + 1.0)
    if warmup_iters and it < warmup_iters:
        k = (1.0 - it / warmup_iters) * (1.0 - warmup_ratio)
        lr = lr * (1.0 - k)
    return lr


def onecycle_beta1(it: int, max_iters: int, base_momentum: float = 0.85, max_momentum: float = 0.95,
                   pct_start: float = 0.3) -> float:
    """mmcv 1.x OneCycleMomentumUpdaterHook with its defaults (cosine annealing, two phases) for an Adam-type optimiser:
    betas[0] goes max -> base over iterations [0, pct_start max_iters - 1], then base -> max up to max_iters - 1."""
    def cos(start, end, pct):
        return end + 0.5 * (start - end) * (math.cos(math.pi * pct) + 1.0)
    e1 = float(pct_start * max_iters) - 1.0
    e2 = float(max_iters - 1)
    if it <= e1:
        return cos(max_momentum, base_momentum, it / e1 if e1 > 0 else 1.0)
    return cos(base_momentum, max_momentum, min(1.0, (it - e1) / (e2 - e1)) if e2 > e1 else 1.0)


def summarize(table: np.ndarray) -> dict:
    """pre_eval_to_metrics: the nanmean over the images of each of the nine per-image metrics ([n, 9] -> dict)."""
    table = np.asarray(table, np.float64).reshape(-1, len(METRICS))
    out = {}
    for i, name in enumerate(METRICS):
        col = table[:, i]
        out[name] = float(np.mean(col[~np.isnan(col)])) if (~np.isnan(col)).any() else float("nan")
    return out


def state_dict_shapes(C_: int, K: int = 256) -> dict:
    """The reference's names and shapes of the head's state dict (the frozen backbone contributes no keys)."""
    return {"decode_head.conv_depth.weight": (K, 2 * C_, 1, 1), "decode_head.conv_depth.bias": (K,)}


def param_layout(C_: int, K: int = 256) -> tuple:
    out = (C.c_int64 * 3)()
    _lib.check(_lib.lib().dvt_depth_param_offsets(C_, K, out), "dvt_depth_param_offsets")
    return int(out[2]), {"conv_depth.weight": (int(out[0]), (K, 2 * C_)), "conv_depth.bias": (int(out[1]), (K,))}


# ================================================================================================ the head
class DepthHeadEngine(FlatAdamW):
    """The depth BNHead on the device.  Features NHWC fp32 [B, h, w, C], cls fp32 [B, C], ground truth fp32 [B, H, W]
    (0 = invalid).  `adamw_step` is one group over both head tensors: no paramwise key of the config matches them."""
    WEIGHT_DECAY = 0.01  # the config's optimizer.weight_decay

    def __init__(self, in_channels: int, device, n_bins: int = 256, min_depth: float = 1e-3, max_depth: float = 10.0,
                 upsample: int = 4, seed: int | None = 0):
        if torch.device(device).type != "cuda":
            raise _lib.DvtError("the depth head needs a HIP device; there is no CPU fallback")
        self.C, self.K, self.up = int(in_channels), int(n_bins), int(upsample)
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)
        super().__init__(*param_layout(self.C, self.K), device)
        self.off_b = self.layout["conv_depth.bias"][0]
        z = lambda n: torch.zeros(n, device=self.device, dtype=torch.float32)  # noqa: E731
        self.bins = torch.linspace(self.min_depth, self.max_depth, self.K, dtype=torch.float32).to(self.device)
        self.out, self.clip_out = z(2), z(2)
        self._clip_work = z(int(_lib.lib().dvt_depth_clip_work_floats(self.total)))
        self._eval_work = None
        self.init_parameters(seed)

    # ---- parameters -------------------------------------------------------------------------------
    def init_parameters(self, seed: int | None = 0) -> None:
        """torch's Conv2d default (the reference's head defines no init of its own): U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
        for weight and bias, fan_in = 2 C."""
        g = torch.Generator().manual_seed(seed) if seed is not None else None
        bound = 1.0 / math.sqrt(2 * self.C)
        v = self.views()
        v["conv_depth.weight"].copy_((torch.rand(self.K, 2 * self.C, generator=g) * 2 - 1) * bound)
        v["conv_depth.bias"].copy_((torch.rand(self.K, generator=g) * 2 - 1) * bound)

    def state_dict(self) -> dict:
        v = self.views()
        return {"decode_head.conv_depth.weight": v["conv_depth.weight"].detach().cpu().reshape(self.K, 2 * self.C, 1, 1).clone(),
                "decode_head.conv_depth.bias": v["conv_depth.bias"].detach().cpu().clone()}

    def load_state_dict(self, sd: dict) -> None:
        for name, shape in state_dict_shapes(self.C, self.K).items():
            if tuple(sd[name].shape) != shape:
                raise ValueError(f"{name}: shape {tuple(sd[name].shape)}, expected {shape}")
        v = self.views()
        v["conv_depth.weight"].copy_(sd["decode_head.conv_depth.weight"].reshape(self.K, 2 * self.C))
        v["conv_depth.bias"].copy_(sd["decode_head.conv_depth.bias"])

    # ---- kernels ----------------------------------------------------------------------------------
    def _check(self, feats: torch.Tensor, cls: torch.Tensor) -> None:
        _lib.require_cuda(feats, cls)
        if feats.dtype != torch.float32 or not feats.is_contiguous() or feats.dim() != 4 or feats.shape[-1] != self.C:
            raise _lib.DvtError(f"features must be contiguous fp32 [B, h, w, {self.C}], got {tuple(feats.shape)} {feats.dtype}")
        if cls.dtype != torch.float32 or not cls.is_contiguous() or tuple(cls.shape) != (feats.shape[0], self.C):
            raise _lib.DvtError(f"cls must be contiguous fp32 [{feats.shape[0]}, {self.C}], got {tuple(cls.shape)} {cls.dtype}")

    def _step_workspace(self, B: int, h: int, w: int, H: int, W: int) -> torch.Tensor:
        nb = int(_lib.lib().dvt_depth_workspace_bytes(B, h, w, self.C, self.K, self.up, H, W))
        if nb <= 0:
            raise _lib.DvtError(f"dvt_depth_workspace_bytes: invalid shape (batch {B}, {h} x {w} tokens, labels {H} x {W})")
        return self._workspace(nb)

    def train_step(self, feats: torch.Tensor, cls: torch.Tensor, depth_gt: torch.Tensor, it: int) -> torch.Tensor:
        """One training step of the head at global iteration `it` (SigLoss warms up while it < 100): writes `grads`;
        -> device [loss_depth, loss_grad] (no synchronisation).  A batch without a valid pixel gives a NaN loss_depth and
        zero gradients."""
        self._check(feats, cls)
        _lib.require_cuda(depth_gt)
        B, h, w, _ = feats.shape
        if depth_gt.dtype != torch.float32 or depth_gt.dim() != 3 or depth_gt.shape[0] != B or not depth_gt.is_contiguous():
            raise _lib.DvtError(f"depth_gt must be contiguous fp32 [{B}, H, W], got {tuple(depth_gt.shape)} {depth_gt.dtype}")
        H, W = depth_gt.shape[1:]
        work = self._step_workspace(B, h, w, H, W)
        _lib.check(_lib.lib().dvt_depth_train_step(
            _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.bins), _lib.ptr(feats), _lib.ptr(cls),
            _lib.ptr(depth_gt), B, h, w, self.C, self.K, self.up, H, W, int(it < WARM_ITERS), GRAD_LOSS_WEIGHT,
            _lib.ptr(work), work.numel(), _lib.ptr(self.out), _lib.stream()), "dvt_depth_train_step")
        return self.out

    def clip_grad_norm(self, max_norm: float) -> torch.Tensor:
        """torch.nn.utils.clip_grad_norm_ over the gradient arena, on the device: -> device [norm, factor]."""
        _lib.check(_lib.lib().dvt_depth_clip_grad_norm(_lib.ptr(self.grads), self.total, float(max_norm),
                                                       _lib.ptr(self._clip_work), _lib.ptr(self.clip_out), _lib.stream()),
                   "dvt_depth_clip_grad_norm")
        return self.clip_out

    def forward(self, feats: torch.Tensor, cls: torch.Tensor) -> torch.Tensor:
        """The head's depth [B, up h, up w] (not clamped)."""
        self._check(feats, cls)
        B, h, w, _ = feats.shape
        depth = torch.empty(B, self.up * h, self.up * w, device=self.device)
        work = self._step_workspace(B, h, w, 0, 0)
        _lib.check(_lib.lib().dvt_depth_forward(_lib.ptr(self.params), _lib.ptr(self.bins), _lib.ptr(feats), _lib.ptr(cls),
                                                B, h, w, self.C, self.K, self.up, _lib.ptr(depth), _lib.ptr(work),
                                                work.numel(), _lib.stream()), "dvt_depth_forward")
        return depth

    def evaluate_maps(self, d0: torch.Tensor, d1: torch.Tensor | None, gt: torch.Tensor, row: torch.Tensor,
                      crop: tuple | None = EIGEN_CROP, want_pred: bool = False):
        """Depth maps of an image (d0) and of its horizontal flip (d1, or None): clamp, resize to gt's size, un-flip,
        average, and the nine metrics over min_depth < gt < max_depth inside `crop` into row [9] (fp64, device)."""
        _lib.require_cuda(d0, d1, gt, row)
        oh, ow = gt.shape
        if gt.dtype != torch.float32 or not gt.is_contiguous() or row.dtype != torch.float64 or row.numel() != len(METRICS):
            raise _lib.DvtError("gt must be contiguous fp32 [H, W] and row fp64 [9]")
        for d in (d0, d1):
            if d is not None and (d.dtype != torch.float32 or not d.is_contiguous() or d.shape != d0.shape or d.dim() != 2):
                raise _lib.DvtError("depth maps must be contiguous fp32 [uh, uw]")
        y0, y1, x0, x1 = crop if crop is not None else (0, oh, 0, ow)
        pred = torch.empty(oh, ow, device=self.device) if want_pred else None
        nb = int(_lib.lib().dvt_depth_eval_work_bytes(oh, ow))
        if self._eval_work is None or self._eval_work.numel() < nb:
            self._eval_work = torch.empty(nb, device=self.device, dtype=torch.uint8)
        work = self._eval_work
        _lib.check(_lib.lib().dvt_depth_eval_image(_lib.ptr(d0), _lib.ptr(d1), d0.shape[0], d0.shape[1], _lib.ptr(gt), oh, ow,
                                                   self.min_depth, self.max_depth, y0, y1, x0, x1, _lib.ptr(pred),
                                                   _lib.ptr(row), _lib.ptr(work), _lib.stream()), "dvt_depth_eval_image")
        return pred

    def evaluate_image(self, img: torch.Tensor, gt: torch.Tensor, row: torch.Tensor, backbone,
                       crop: tuple | None = EIGEN_CROP, flip: bool = True, want_pred: bool = False):
        """The reference's test of one normalised image [3, H, W]: the image and its horizontal flip through `backbone(batch)
        -> (features [n, h, w, C], cls [n, C])` and the head, then evaluate_maps against gt [H, W]."""
        _lib.require_cuda(img)
        batch = torch.stack([img, img.flip(-1)]) if flip else img[None]
        feats, cls = backbone(batch.contiguous())
        d = self.forward(feats.contiguous(), cls.contiguous())
        return self.evaluate_maps(d[0], d[1] if flip else None, gt, row, crop, want_pred)
