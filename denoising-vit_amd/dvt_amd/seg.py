"""Host side of the linear-probe segmentation evaluation (csrc/dvt_seg.hip, C ABI in include/dvt_seg.h).

The reference evaluates denoised features with `evaluate_dense_tasks.py --task segmentation` and the linear configs: mmseg
0.27's `BNHead` (SyncBatchNorm, then `conv_seg`, a 1 x 1 convolution to the classes) trained on frozen backbone features,
then slide inference and mIoU.  `SegHeadEngine` owns that head: flat fp32 parameter / gradient / AdamW-moment arenas (layout
of `dvt_seg_param_offsets`, stepped by `dvt_adamw_step`) and the running statistics.  `train_step` is one step of the head
on a batch of features (BN statistics, logits, upsampled CE, every parameter gradient), `slide_inference` / `evaluate_image`
are mmseg's EncoderDecoder.slide_inference and the intersect_and_union histograms.

The pure host pieces of the evaluation (the LR schedule, the slide-window grid, DINOv2's centre padding, the metrics and
the checkpoint layout) are plain Python here, so that they can be checked without a GPU.
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
    "dvt_seg_param_offsets": (_I, [_I, _I, C.POINTER(C.c_int64)]),
    "dvt_seg_stats_parts": (_I, [_I64]),
    "dvt_seg_workspace_bytes": (_I64, [_I, _I, _I, _I, _I, _I, _I]),
    "dvt_seg_bn_stats": (_I, [_P, _I64, _I, _P, _P, _P]),
    "dvt_seg_bn_merge": (_I, [_P, _I, _I, _P, _P]),
    "dvt_seg_train_step": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _F, _P, _I64, _P, _P]),
    "dvt_seg_forward": (_I, [_P, _P, _P, _I64, _I, _I, _F, _P, _P, _I64, _P]),
    "dvt_seg_slide_accum": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _I, _I, _P]),
    "dvt_seg_finalize": (_I, [_P, _P, _I, _I, _I, _P, _I, _I, _I, _P, _P, _P]),
})

IGNORE_INDEX = 255
BN_MOMENTUM = 0.1
BN_EPS = 1e-5


# ================================================================================================ pure host pieces
def poly_lr(it: int, base_lr: float, max_iters: int, power: float = 1.0, min_lr: float = 0.0,
            warmup_iters: int = 1500, warmup_ratio: float = 1e-6) -> float:
    """mmcv's PolyLrUpdaterHook (by_epoch=False) with linear warmup, at 0-based iteration `it`."""
    coeff = (1.0 - it / max_iters) ** power
    lr = (base_lr - min_lr) * coeff + min_lr
    if warmup_iters and it < warmup_iters:
        k = (1.0 - it / warmup_iters) * (1.0 - warmup_ratio)
        lr = lr * (1.0 - k)
    return lr


def slide_windows(h_img: int, w_img: int, crop: tuple = (512, 512), stride: tuple = (341, 341)) -> list:
    """mmseg EncoderDecoder.slide_inference's crop boxes, in its order: [(y1, y2, x1, x2), ...]."""
    (h_crop, w_crop), (h_stride, w_stride) = crop, stride
    h_grids = max(h_img - h_crop + h_stride - 1, 0) // h_stride + 1
    w_grids = max(w_img - w_crop + w_stride - 1, 0) // w_stride + 1
    boxes = []
    for hi in range(h_grids):
        for wi in range(w_grids):
            y1, x1 = hi * h_stride, wi * w_stride
            y2, x2 = min(y1 + h_crop, h_img), min(x1 + w_crop, w_img)
            boxes.append((max(y2 - h_crop, 0), y2, max(x2 - w_crop, 0), x2))
    return boxes


def center_pad(size: int, multiple: int) -> tuple:
    """DINOv2's CenterPadding for one side length: (left, right) zero padding up to a multiple of the patch size."""
    pad = math.ceil(size / multiple) * multiple - size
    return pad // 2, pad - pad // 2


def total_area_to_metrics(hist: np.ndarray) -> dict:
    """mmseg 0.27 total_area_to_metrics(metrics=['mIoU']) from hist [3, K] = (intersect, pred, label) areas; the summary
    values are nanmean over the classes (a class absent from both prediction and label is NaN and does not count)."""
    inter, pred, label = (np.asarray(h, np.float64) for h in hist)
    union = pred + label - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / union
        acc = inter / label
        aacc = inter.sum() / label.sum()
    return {"aAcc": float(aacc), "IoU": iou, "Acc": acc, "mIoU": float(np.nanmean(iou)) if np.isfinite(iou).any()
            else float("nan"), "mAcc": float(np.nanmean(acc)) if np.isfinite(acc).any() else float("nan")}


def param_layout(C_: int, K: int) -> tuple:
    out = (C.c_int64 * 5)()
    _lib.check(_lib.lib().dvt_seg_param_offsets(C_, K, out), "dvt_seg_param_offsets")
    o = [int(v) for v in out]
    return o[4], {"conv_seg.weight": (o[0], (K, C_)), "conv_seg.bias": (o[1], (K,)),
                  "bn.weight": (o[2], (C_,)), "bn.bias": (o[3], (C_,))}


def state_dict_shapes(C_: int, K: int) -> dict:
    """mmseg's names and shapes of the head's state dict (the backbone contributes no keys)."""
    return {"decode_head.conv_seg.weight": (K, C_, 1, 1), "decode_head.conv_seg.bias": (K,),
            "decode_head.bn.weight": (C_,), "decode_head.bn.bias": (C_,), "decode_head.bn.running_mean": (C_,),
            "decode_head.bn.running_var": (C_,), "decode_head.bn.num_batches_tracked": ()}


# ================================================================================================ the head
class SegHeadEngine(FlatAdamW):
    """BNHead + conv_seg on the device.  Features are NHWC fp32 [B, h, w, C]; labels uint8 [B, H, W] (255 ignored).
    `adamw_step` is one group over every head tensor, as mmcv builds it from the config."""
    WEIGHT_DECAY = 1e-4  # the linear configs' optimizer.weight_decay

    def __init__(self, in_channels: int, num_classes: int, device, seed: int | None = 0):
        if torch.device(device).type != "cuda":
            raise _lib.DvtError("the segmentation head needs a HIP device; there is no CPU fallback")
        self.C, self.K = int(in_channels), int(num_classes)
        super().__init__(*param_layout(self.C, self.K), device)
        z = lambda n: torch.zeros(n, device=self.device, dtype=torch.float32)  # noqa: E731
        self.running = torch.cat([z(self.C), torch.ones(self.C, device=self.device)])
        self.num_batches_tracked = 0
        self.out = z(2)
        self.init_parameters(seed)

    # ---- parameters -------------------------------------------------------------------------------
    def init_parameters(self, seed: int | None = 0) -> None:
        """mmseg's init: conv_seg ~ N(0, 0.01^2), bias 0; BN weight 1, bias 0."""
        g = torch.Generator().manual_seed(seed) if seed is not None else None
        v = self.views()
        self.params.zero_()
        v["conv_seg.weight"].copy_(torch.randn(self.K, self.C, generator=g) * 0.01)
        v["bn.weight"].fill_(1.0)

    def state_dict(self) -> dict:
        v = self.views()
        return {"decode_head.conv_seg.weight": v["conv_seg.weight"].detach().cpu().reshape(self.K, self.C, 1, 1).clone(),
                "decode_head.conv_seg.bias": v["conv_seg.bias"].detach().cpu().clone(),
                "decode_head.bn.weight": v["bn.weight"].detach().cpu().clone(),
                "decode_head.bn.bias": v["bn.bias"].detach().cpu().clone(),
                "decode_head.bn.running_mean": self.running[:self.C].cpu().clone(),
                "decode_head.bn.running_var": self.running[self.C:].cpu().clone(),
                "decode_head.bn.num_batches_tracked": torch.tensor(self.num_batches_tracked, dtype=torch.int64)}

    def load_state_dict(self, sd: dict) -> None:
        v = self.views()
        for name, t in self.state_dict().items():
            if tuple(sd[name].shape) != tuple(t.shape):
                raise ValueError(f"{name}: shape {tuple(sd[name].shape)}, expected {tuple(t.shape)}")
        v["conv_seg.weight"].copy_(sd["decode_head.conv_seg.weight"].reshape(self.K, self.C))
        v["conv_seg.bias"].copy_(sd["decode_head.conv_seg.bias"])
        v["bn.weight"].copy_(sd["decode_head.bn.weight"])
        v["bn.bias"].copy_(sd["decode_head.bn.bias"])
        self.running[:self.C].copy_(sd["decode_head.bn.running_mean"])
        self.running[self.C:].copy_(sd["decode_head.bn.running_var"])
        self.num_batches_tracked = int(sd["decode_head.bn.num_batches_tracked"])

    # ---- kernels ----------------------------------------------------------------------------------
    def _check_feats(self, feats: torch.Tensor) -> None:
        _lib.require_cuda(feats)
        if feats.dtype != torch.float32 or not feats.is_contiguous() or feats.dim() != 4 or feats.shape[-1] != self.C:
            raise _lib.DvtError(f"features must be contiguous fp32 [B, h, w, {self.C}], got {tuple(feats.shape)} "
                                f"{feats.dtype}")

    def batch_stats(self, feats: torch.Tensor) -> torch.Tensor:
        """This batch's statistics record [3 C + 4] = (mean_hi, mean_lo, M2, count, 0, 0, 0): what SyncBN gathers across ranks."""
        self._check_feats(feats)
        n = feats.numel() // self.C
        P = _lib.lib().dvt_seg_stats_parts(n)
        parts = torch.empty(P * (3 * self.C + 4), device=self.device)
        stats = torch.empty(3 * self.C + 4, device=self.device)
        _lib.check(_lib.lib().dvt_seg_bn_stats(_lib.ptr(feats), n, self.C, _lib.ptr(parts), _lib.ptr(stats),
                                               _lib.stream()), "dvt_seg_bn_stats")
        return stats

    def merge_stats(self, records: torch.Tensor) -> torch.Tensor:
        """Merge [n, 3 C + 4] records in order (Chan's rule) into one."""
        records = records.contiguous()
        out = torch.empty(3 * self.C + 4, device=self.device)
        _lib.check(_lib.lib().dvt_seg_bn_merge(_lib.ptr(records), records.shape[0], self.C, _lib.ptr(out),
                                               _lib.stream()), "dvt_seg_bn_merge")
        return out

    def train_step(self, feats: torch.Tensor, labels: torch.Tensor, stats: torch.Tensor | None = None) -> torch.Tensor:
        """One training step of the head: writes `grads`, updates the running statistics; -> device [loss, acc_seg]
        (no synchronisation).  `stats`: the merged record of every rank (SyncBN), None for this batch's own."""
        self._check_feats(feats)
        _lib.require_cuda(labels)
        B, h, w, _ = feats.shape
        if labels.dtype != torch.uint8 or labels.dim() != 3 or labels.shape[0] != B or not labels.is_contiguous():
            raise _lib.DvtError(f"labels must be contiguous uint8 [{B}, H, W], got {tuple(labels.shape)} {labels.dtype}")
        H, W = labels.shape[1:]
        nb = int(_lib.lib().dvt_seg_workspace_bytes(B, h, w, self.C, self.K, H, W))
        if nb <= 0:
            raise _lib.DvtError("dvt_seg_workspace_bytes: invalid shape")
        work = self._workspace(nb)
        _lib.check(_lib.lib().dvt_seg_train_step(
            _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.running), _lib.ptr(feats), _lib.ptr(labels),
            _lib.ptr(stats), B, h, w, self.C, self.K, H, W, BN_MOMENTUM, BN_EPS, _lib.ptr(work), work.numel(),
            _lib.ptr(self.out), _lib.stream()), "dvt_seg_train_step")
        self.num_batches_tracked += 1
        return self.out

    def forward(self, feats: torch.Tensor) -> torch.Tensor:
        """Inference head (running statistics): logits [B, h, w, K]."""
        self._check_feats(feats)
        B, h, w, _ = feats.shape
        z = torch.empty(B, h, w, self.K, device=self.device)
        work = self._workspace(int(_lib.lib().dvt_seg_workspace_bytes(1, 1, 1, self.C, self.K, 0, 0)))
        _lib.check(_lib.lib().dvt_seg_forward(_lib.ptr(self.params), _lib.ptr(self.running), _lib.ptr(feats), B * h * w,
                                              self.C, self.K, BN_EPS, _lib.ptr(z), _lib.ptr(work), work.numel(),
                                              _lib.stream()), "dvt_seg_forward")
        return z

    def slide_inference(self, img: torch.Tensor, backbone, crop=(512, 512), stride=(341, 341)):
        """mmseg EncoderDecoder.slide_inference for one normalised image [3, H, W] (fp32, device): -> (canvas [K, H, W],
        count [H, W]) before the division.  `backbone(batch [n, 3, ch, cw]) -> [n, h, w, C]` features; the crops of one
        size go through the backbone as one batch."""
        _lib.require_cuda(img)
        _, H, W = img.shape
        canvas = torch.zeros(self.K, H, W, device=self.device)
        count = torch.zeros(H, W, device=self.device)
        boxes = slide_windows(H, W, crop, stride)
        crops = torch.stack([img[:, y1:y2, x1:x2] for (y1, y2, x1, x2) in boxes]).contiguous()
        z = self.forward(backbone(crops).contiguous())
        _, h, w, _ = z.shape
        for i, (y1, y2, x1, x2) in enumerate(boxes):
            _lib.check(_lib.lib().dvt_seg_slide_accum(_lib.ptr(z[i]), h, w, self.K, y2 - y1, x2 - x1, y1, x1,
                                                      _lib.ptr(canvas), _lib.ptr(count), H, W, _lib.stream()),
                       "dvt_seg_slide_accum")
        return canvas, count

    def finalize(self, canvas: torch.Tensor, count: torch.Tensor, out_size: tuple, label: torch.Tensor | None = None,
                 hist: torch.Tensor | None = None, reduce_zero_label: bool = False, want_pred: bool = False):
        """canvas / count resized to `out_size`, argmax, and (with `label` [oh, ow] uint8) hist [3, K] int64 +=
        (area_intersect, area_pred, area_label).  -> the prediction [oh, ow] int32 if `want_pred`."""
        K, H, W = canvas.shape
        oh, ow = out_size
        pred = torch.empty(oh, ow, device=self.device, dtype=torch.int32) if want_pred else None
        if label is not None:
            _lib.require_cuda(label, hist)
            if label.dtype != torch.uint8 or tuple(label.shape) != (oh, ow) or not label.is_contiguous():
                raise _lib.DvtError(f"label must be contiguous uint8 [{oh}, {ow}]")
            if hist is None or hist.dtype != torch.int64 or tuple(hist.shape) != (3, K):
                raise _lib.DvtError(f"hist must be int64 [3, {K}]")
        _lib.check(_lib.lib().dvt_seg_finalize(_lib.ptr(canvas), _lib.ptr(count), K, H, W, _lib.ptr(label), oh, ow,
                                               int(reduce_zero_label), _lib.ptr(hist), _lib.ptr(pred), _lib.stream()),
                   "dvt_seg_finalize")
        return pred

    def evaluate_image(self, img: torch.Tensor, label: torch.Tensor, hist: torch.Tensor, backbone,
                       reduce_zero_label: bool = False, crop=(512, 512), stride=(341, 341)) -> None:
        """Slide inference on the test-resized image, resize to the label's (original) size, histograms into `hist`."""
        canvas, count = self.slide_inference(img, backbone, crop, stride)
        self.finalize(canvas, count, tuple(label.shape), label, hist, reduce_zero_label)


# ================================================================================================ backbones
class ViTBackbone:
    """Frozen DINOv2 ViT as mmseg's backbone in the linear configs: the input is zero-padded to a multiple of the patch
    size, centred (CenterPadding), and the last block's final-normed patch tokens are the features (in_index [3] of
    out_indices [8, 9, 10, 11] is the last block).  One HipViT per padded input size, a few kept."""
    CACHE = 4

    def __init__(self, state_dict: dict, patch: int, device, dtype: str = "bfloat16", denoiser=None,
                 return_cls: bool = False):
        """return_cls: the call returns (features, cls [B, C]): the final-normed cls token of the ViT beside the features (the
        depth probe's input; with a denoiser the features are the denoiser's and the cls token stays the ViT's own)."""
        self.sd, self.patch, self.device, self.dtype, self.denoiser = state_dict, patch, torch.device(device), dtype, denoiser
        self.return_cls = return_cls
        self._engines = {}

    def _engine(self, hp: int, wp: int):
        from .vit import HipViT
        key = (hp, wp)
        if key in self._engines:
            self._engines[key] = self._engines.pop(key)
        else:
            while len(self._engines) >= self.CACHE:
                self._engines.pop(next(iter(self._engines)))
            self._engines[key] = HipViT(self.sd, self.patch, self.patch, (hp, wp), self.device, dtype=self.dtype)
        return self._engines[key]

    def __call__(self, img: torch.Tensor):
        _, _, H, W = img.shape
        (t, b), (l, r) = center_pad(H, self.patch), center_pad(W, self.patch)
        x = torch.nn.functional.pad(img, (l, r, t, b)).contiguous()
        cls = None
        with torch.no_grad():
            f = self._engine(H + t + b, W + l + r).forward_features(x.float(), return_cls=self.return_cls)
            if self.return_cls:
                f, cls = f
            if self.denoiser is not None:
                f = self.denoiser(f.contiguous())
        return (f.contiguous(), cls) if self.return_cls else f.contiguous()
