"""Host side of the stage-3 distillation step (csrc/dvt_stage3.hip, C ABI in include/dvt_stage3.h).

`Stage3Engine` owns four flat fp32 arenas on the device -- parameters, gradients and the two AdamW moments of a whole
DINOv2 ViT, in the layout `dvt_s3_param_offsets` reports, every tensor under its timm name and shape -- plus the
activation workspace.  `train_step` is forward + loss + backward of the student (main_distillation.py: the wrapper's
get_intermediate_layers(n=1, norm=True) features against the teacher's), gradients accumulated into `grads`; a batch
larger than the workspace budget runs in slices whose loss terms are normalised by the whole batch, so the accumulated
gradient is the whole batch's.  `adamw_step` is torch.optim.AdamW over the flat arenas (dvt_adamw_step).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .arena import FlatAdamW
from .vit import VitConfig, vit_config

BLOCK_TENSORS = ["norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                 "ls1.gamma", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
                 "mlp.fc2.bias", "ls2.gamma"]

_P, _I = C.c_void_p, C.c_int
_lib.register_signatures({
    "dvt_s3_param_offsets": (_I, [C.POINTER(VitConfig), C.POINTER(C.c_int64)]),
    "dvt_s3_workspace_bytes": (C.c_int64, [C.POINTER(VitConfig), _I]),
    "dvt_s3_train_step": (_I, [C.POINTER(VitConfig), _P, _P, _P, _P, _P, _I, _P, C.c_int64, _P, _P]),
    "dvt_s3_train_slice": (_I, [C.POINTER(VitConfig), _P, _P, _P, _P, _P, _I, _I, _P, C.c_int64, _P, _P]),
})


def make_config(dim: int, depth: int, patch: int, stride: int, img_h: int, img_w: int, n_reg: int = 0) -> VitConfig:
    if dim not in (384, 768, 1024):
        raise NotImplementedError(f"the stage-3 step is built for dim 384 / 768 / 1024, got {dim}")
    return vit_config(dim, depth, patch, stride, img_h, img_w, n_reg, row_pad=128)


def tensor_shapes(cfg: VitConfig) -> list:
    """Shapes of the timm tensors in arena order (names: `param_layout`)."""
    d, f, p = cfg.dim, cfg.mlp_dim, cfg.patch
    block = [(d,), (d,), (3 * d, d), (3 * d,), (d, d), (d,), (d,), (d,), (d,), (f, d), (f,), (d, f), (d,), (d,)]
    return ([(d, 3, p, p), (d,), (1, 1, d), (1, cfg.n_prefix - 1, d), (1, cfg.pos_has_cls + cfg.grid_h * cfg.grid_w, d)]
            + block * cfg.depth + [(d,), (d,)])


def param_names(cfg: VitConfig) -> list:
    return (["patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token", "reg_token", "pos_embed"]
            + [f"blocks.{b}.{t}" for b in range(cfg.depth) for t in BLOCK_TENSORS] + ["norm.weight", "norm.bias"])


def param_layout(cfg: VitConfig):
    """-> (total floats, {timm name: (offset, shape)}); `reg_token` only for models with register tokens."""
    n = 8 + 14 * cfg.depth
    out = (C.c_int64 * n)()
    _lib.check(_lib.lib().dvt_s3_param_offsets(C.byref(cfg), out), "dvt_s3_param_offsets")
    layout = {}
    for i, (name, shape) in enumerate(zip(param_names(cfg), tensor_shapes(cfg))):
        if name == "reg_token" and cfg.n_prefix == 1:
            continue
        layout[name] = (int(out[i]), shape)
    return int(out[n - 1]), layout


class Stage3Engine(FlatAdamW):
    def __init__(self, cfg: VitConfig, device: torch.device, max_work_bytes: int | None = None):
        """`max_work_bytes`: budget of the activation workspace (default: 80 % of the device memory free after the
        arenas are allocated); `train_step` splits a batch into slices that fit."""
        if torch.device(device).type != "cuda":
            raise _lib.DvtError("the stage-3 engine needs a HIP device; there is no CPU fallback")
        self.cfg = cfg
        super().__init__(*param_layout(cfg), device)
        self.loss = torch.zeros(4, device=self.device, dtype=torch.float32)
        self._slice_loss = torch.zeros(4, device=self.device, dtype=torch.float32)
        self.max_work_bytes = max_work_bytes

    # ---- parameters -------------------------------------------------------------------------------
    def load_timm(self, state: dict) -> None:
        """Copy a timm VisionTransformer state dict (DINOv2 layout) into the parameter arena.  Only the checkpoint's own
        position grid is trained: another grid would need the pos_embed resample's backward."""
        v = self.views()
        missing = [k for k in v if k not in state]
        if missing:
            raise KeyError(f"ViT state dict lacks {missing}")
        for k, dst in v.items():
            src = state[k]
            if k == "pos_embed" and tuple(src.shape) != tuple(dst.shape):
                raise NotImplementedError(
                    f"pos_embed {tuple(src.shape)} is not the trained grid {tuple(dst.shape)}: the stage-3 step trains the "
                    "checkpoint's own position grid only (the pos_embed resample backward is not built)")
            dst.copy_(src.detach().to(self.device, torch.float32).reshape(dst.shape))

    def state_dict(self) -> dict:
        """timm names -> CPU fp32 tensors (copies)."""
        return {k: t.detach().cpu().clone() for k, t in self.views().items()}

    # ---- kernels ----------------------------------------------------------------------------------
    def workspace_bytes(self, batch: int) -> int:
        n = int(_lib.lib().dvt_s3_workspace_bytes(C.byref(self.cfg), batch))
        if n <= 0:
            raise _lib.DvtError("dvt_s3_workspace_bytes: invalid configuration")
        return n

    def slice_size(self, batch: int) -> int:
        """Images per slice for a batch of `batch`: the largest count whose workspace fits the budget."""
        budget = self.max_work_bytes
        if budget is None:
            free, _ = torch.cuda.mem_get_info(self.device)
            budget = int(0.8 * free) + (self._work.numel() if self._work is not None else 0)
        need = self.workspace_bytes(1)
        if need > budget:
            raise _lib.DvtError(f"one image needs {need} bytes of stage-3 workspace, {budget} are available")
        b = batch
        while b > 1 and self.workspace_bytes(b) > budget:
            b = max(1, min(b - 1, budget // need))
        return b

    def _check(self, img: torch.Tensor, target: torch.Tensor, feat: torch.Tensor | None):
        _lib.require_cuda(img, target, feat)
        c = self.cfg
        if img.dtype != torch.float32 or not img.is_contiguous() or tuple(img.shape[1:]) != (3, c.img_h, c.img_w):
            raise _lib.DvtError(f"expected a contiguous fp32 image batch [B, 3, {c.img_h}, {c.img_w}], got "
                                f"{tuple(img.shape)} {img.dtype}")
        want = (img.shape[0], c.grid_h, c.grid_w, c.dim)
        for name, t in (("target", target), ("feat", feat)):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != want):
                raise _lib.DvtError(f"{name} must be a contiguous fp32 {list(want)} tensor, got {tuple(t.shape)} {t.dtype}")

    def train_step(self, img: torch.Tensor, target: torch.Tensor, feat: torch.Tensor | None = None,
                   micro_batch: int | None = None) -> torch.Tensor:
        """Gradients of this batch are ADDED to `self.grads`; returns the device tensor [loss, l2_loss,
        cosine_similarity_loss, 0] of the whole batch (no synchronisation).  `feat` receives the student features.
        `micro_batch`: images per slice (default: as many as the workspace budget allows)."""
        self._check(img, target, feat)
        B = img.shape[0]
        mb = self.slice_size(B) if micro_batch is None else max(1, min(int(micro_batch), B))
        w = self._workspace(self.workspace_bytes(mb))
        L = _lib.lib()
        if mb >= B:
            _lib.check(L.dvt_s3_train_step(C.byref(self.cfg), _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(img),
                                           _lib.ptr(target), _lib.ptr(feat), B, _lib.ptr(w), w.numel(),
                                           _lib.ptr(self.loss), _lib.stream()), "dvt_s3_train_step")
            return self.loss
        l2 = torch.zeros((), device=self.device)
        cos = torch.zeros((), device=self.device)
        for b0 in range(0, B, mb):
            n = min(mb, B - b0)
            _lib.check(L.dvt_s3_train_slice(C.byref(self.cfg), _lib.ptr(self.params), _lib.ptr(self.grads),
                                            _lib.ptr(img[b0:]), _lib.ptr(target[b0:]),
                                            None if feat is None else _lib.ptr(feat[b0:]), n, B, _lib.ptr(w), w.numel(),
                                            _lib.ptr(self._slice_loss), _lib.stream()), "dvt_s3_train_slice")
            l2 += self._slice_loss[1]
            cos += 1.0 - self._slice_loss[2]
        self.loss.copy_(torch.stack([l2 + 1.0 - cos, l2, 1.0 - cos, torch.zeros_like(l2)]))
        return self.loss
