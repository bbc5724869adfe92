"""`Denoiser` -- the stage-2 generalizable denoiser behind the reference's class
(dvt/models/online_denoiser.py:13-104): same constructor arguments, same `forward` keywords and result keys,
same state-dict names (`pos_embed`, `denoiser.norm1.weight`, `denoiser.attn.qkv.weight`, ...; `denoiser.<i>.`
for num_blocks > 1), so checkpoints written by main_denoiser.py:239-251 (`{"denoiser": state_dict}`) load
unchanged.  Every parameter is a view into ONE flat device arena owned by `dvt_amd.s2.Stage2Engine`; compute is
the HIP library (csrc/dvt_stage2.hip), there is no CPU path.  `inference_dtype="bfloat16"` (opt-in) sends `forward` through
the bf16 extractor's block kernels instead (csrc/dvt_denoiser.hip, dvt_amd/denoiser_bf16.py); parameters, training and
checkpoints stay fp32.

Training differs from the reference in one place: the reference differentiates through autograd
(`loss.backward()`, main_denoiser.py:218-221); here `training_step(original_feats, denoised_feats)` runs
forward + loss + backward natively and leaves the gradients in `engine.grads` for the optimizer step.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import s2
from ..vit import resample_pos_embed
from .vit_wrapper import PretrainedViTWrapper


class _Holder(nn.Module):
    """A parameter container with the attribute path of the timm module it stands for."""


def _attach(root: nn.Module, dotted: str, p: nn.Parameter) -> None:
    parts = dotted.split(".")
    m = root
    for name in parts[:-1]:
        if not hasattr(m, name):
            m.add_module(name, _Holder())
        m = getattr(m, name)
    m.register_parameter(parts[-1], p)


class Denoiser(nn.Module):
    RESIZED_CACHE = 4  # resized inference copies kept (LRU)
    def __init__(self, noise_map_height: int = 37, noise_map_width: int = 37, feat_dim: int = 768,
                 vit: PretrainedViTWrapper = None, enable_pe: bool = True, num_blocks: int = 1,
                 device: torch.device | str = "cuda", seed: int | None = None, inference_dtype: str = "float32",
                 train_dtype: str = "float32", train_attention: str = "float32", train_weight_grad: str = "float32"):
        """train_dtype / train_attention / train_weight_grad: arithmetic of `training_step`, handed to `Stage2Engine` as its
        dtype / attention / weight_grad ("float32" each by default: exact fp32; "bfloat16" opt-in, the last two on top of
        train_dtype="bfloat16" only).  `forward`, `load_state_dict`, the state dict and the checkpoint format do not depend on
        them.
        inference_dtype: arithmetic of `forward`.  "float32" (default): the exact-fp32 forward of the trainer
        (Stage2Engine.forward).  "bfloat16" (opt-in): the bf16 extractor's block kernels (dvt_amd.denoiser_bf16) -- on the
        given features without a `vit`; with one, image in and denoised features out of one launch sequence, for which the
        wrapper must run in bfloat16 too.  Training and the state dict are fp32 either way."""
        super().__init__()
        if inference_dtype not in ("float32", "bfloat16"):
            raise ValueError(f"inference_dtype must be 'float32' or 'bfloat16', not {inference_dtype!r}")
        if inference_dtype == "bfloat16" and vit is not None and vit.dtype != "bfloat16":
            raise ValueError(f"Denoiser(inference_dtype='bfloat16') over a vit with dtype={vit.dtype!r}: the fused forward "
                             "reads the bf16 extractor's residual stream; build the wrapper with dtype='bfloat16' or keep "
                             "inference_dtype='float32'")
        mode = s2.gemm_mode(train_dtype, train_attention, train_weight_grad)  # (refused by name before a device is touched)
        self.inference_dtype = inference_dtype
        self.vit = vit
        self.noise_map_size = (noise_map_height, noise_map_width)
        cfg = s2.make_config(feat_dim, noise_map_height * noise_map_width, num_blocks, enable_pe,
                             row_pad=s2.BF16_ROW_PAD if mode else 64)
        self.engine = s2.Stage2Engine(cfg, torch.device(device), dtype=train_dtype, attention=train_attention,
                                      weight_grad=train_weight_grad)
        g = None if seed is None else torch.Generator().manual_seed(seed)
        self.engine.init_parameters(g)
        # registration order of the reference: denoiser blocks, then pos_embed (online_denoiser.py:24-57)
        self.denoiser = _Holder()
        self.pos_embed = None
        views = self.engine.views()
        for name, v in views.items():
            if name != "pos_embed":
                _attach(self, name, nn.Parameter(v))
        if enable_pe:
            self.pos_embed = nn.Parameter(views["pos_embed"])
        if self.vit is not None:
            for p in self.vit.parameters():
                p.requires_grad = False
        self._resized = {}
        self._resized_version = -1
        self._bf16 = {}  # grid -> HipDenoiser of the current parameter version (inference_dtype="bfloat16")
        self._bf16_version = -1

    # parameters are views of the engine's arena: moving the module must move the arena, not the views
    def _apply(self, fn, recurse=True):
        probe = fn(torch.empty(0, device=self.engine.device))
        if probe.device != self.engine.device or probe.dtype != torch.float32:
            raise NotImplementedError("Denoiser lives on the HIP device it was built on, in fp32 "
                                      "(construct it with device=...)")
        return self

    def load_state_dict(self, state_dict, strict: bool = True):
        sd = {k: v for k, v in state_dict.items() if not k.startswith("vit.")}  # main_denoiser.py:241-245
        self.engine.load_named(sd)
        self._resized.clear()
        self._bf16.clear()
        return nn.modules.module._IncompatibleKeys([], [k for k in sd if k not in self.engine.layout])

    def _engine_for(self, h: int, w: int) -> s2.Stage2Engine:
        """Inference at another token grid: timm's `resample_abs_pos_embed` (online_denoiser.py:89) applied
        once to a copy of the parameters."""
        if (h, w) == self.noise_map_size or self.pos_embed is None and h * w == self.engine.cfg.tokens:
            return self.engine
        # resized copies: parameters only (no gradient / moment arenas), at most RESIZED_CACHE of them (LRU: dense-task
        # evaluation over variable-size inputs must not grow device memory without bound), and valid for ONE parameter
        # version -- any write through the engine (adamw_step, load_named) invalidates them, not only training_step
        if self._resized_version != self.engine.param_version:
            self._resized.clear()
            self._resized_version = self.engine.param_version
        if (h, w) in self._resized:
            self._resized[(h, w)] = self._resized.pop((h, w))  # most recently used last
        if (h, w) not in self._resized:
            while len(self._resized) >= self.RESIZED_CACHE:
                self._resized.pop(next(iter(self._resized)))
            c = self.engine.cfg
            e = s2.Stage2Engine(s2.make_config(c.dim, h * w, c.n_blocks, bool(c.enable_pe)), self.engine.device,
                                inference_only=True)
            src, dst = self.engine.views(), e.views()
            for k in dst:
                if k == "pos_embed":
                    gh, gw = self.noise_map_size
                    dst[k].copy_(resample_pos_embed(src[k].detach().cpu().reshape(1, gh * gw, c.dim), (h, w), 0)
                                 .to(e.device))
                else:
                    dst[k].copy_(src[k])
            self._resized[(h, w)] = e
        return self._resized[(h, w)]

    def _bf16_for(self, h: int, w: int):
        """The bf16 weights at one grid: built from the engine's parameter views, kept under `_engine_for`'s rule -- at most
        RESIZED_CACHE grids (LRU), all dropped when the engine's param_version moves."""
        from ..denoiser_bf16 import HipDenoiser
        if self._bf16_version != self.engine.param_version:
            self._bf16.clear()
            self._bf16_version = self.engine.param_version
        if (h, w) in self._bf16:
            self._bf16[(h, w)] = self._bf16.pop((h, w))  # most recently used last
        else:
            while len(self._bf16) >= self.RESIZED_CACHE:
                self._bf16.pop(next(iter(self._bf16)))
            c = self.engine.cfg
            self._bf16[(h, w)] = HipDenoiser(self.engine.views(), self.noise_map_size, (h, w), c.n_blocks, bool(c.enable_pe),
                                             self.engine.device)
        return self._bf16[(h, w)]

    def _forward_bf16(self, x, return_original: bool, return_class_token: bool, norm: bool):
        """-> (denoised NHWC, original_feats NHWC or None, class_tokens or None) in bf16 arithmetic."""
        if self.vit is None:
            b, h, w, c = x.shape
            return self._bf16_for(h, w).forward(x.float()), x, None
        if not norm:
            raise ValueError("Denoiser(inference_dtype='bfloat16') with norm=False: the fused forward reads the vit's last "
                             "layer through its final LayerNorm (norm=True); use inference_dtype='float32' for norm=False")
        if self.vit.dtype != "bfloat16":
            raise ValueError(f"Denoiser(inference_dtype='bfloat16') over a vit with dtype={self.vit.dtype!r}")
        hip = self.vit._engine(x.device)
        return self._bf16_for(hip.cfg.grid_h, hip.cfg.grid_w).forward_fused(hip, x.float(), return_original=return_original,
                                                                            return_cls=return_class_token)

    def forward(self, x, return_dict=False, return_channel_first=False, return_class_token=False, norm=True):
        class_tokens = None
        # without a ViT there is no class token to return: the reference's assert (online_denoiser.py:101-103), before any work
        assert self.vit is not None or return_dict or not return_class_token, "return_class_token=True needs a vit"
        if self.inference_dtype == "bfloat16":
            with torch.no_grad():
                y, original_feats, class_tokens = self._forward_bf16(x, return_dict, return_class_token, norm)
            if return_channel_first:
                y = y.permute(0, 3, 1, 2)
            if return_dict:
                return {"denoised_feats": y, "original_feats": original_feats.detach(), "class_tokens": class_tokens}
            if return_class_token:
                return y, class_tokens
            return y
        if self.vit is not None:
            with torch.no_grad():  # online_denoiser.py:70-84
                vit_outputs = self.vit.get_intermediate_layers(x, n=[self.vit.last_layer_index],
                                                               return_prefix_tokens=return_class_token, norm=norm)
                if return_class_token:
                    vit_outputs = vit_outputs[-1]
                    class_tokens = vit_outputs[1][:, 0]
                original_feats = vit_outputs[0].permute(0, 2, 3, 1)
                x = original_feats
        else:
            original_feats = x
        b, h, w, c = x.shape
        eng = self._engine_for(h, w)
        with torch.no_grad():
            y = eng.forward(x.reshape(b, h * w, c).contiguous().float()).reshape(b, h, w, c)
        if return_channel_first:
            y = y.permute(0, 3, 1, 2)
        if return_dict:
            return {"denoised_feats": y, "original_feats": original_feats.detach(),
                    "class_tokens": class_tokens.detach() if class_tokens is not None else None}
        if return_class_token:
            return y, class_tokens
        return y

    def training_step(self, original_feats: torch.Tensor, denoised_feats: torch.Tensor,
                      pred: torch.Tensor | None = None) -> torch.Tensor:
        """main_denoiser.py:212-220 in one native call; -> device tensor [loss, l2_loss, cosine_similarity_loss, 0]."""
        b, h, w, c = original_feats.shape
        if (h, w) != self.noise_map_size:
            raise ValueError("training runs at the noise-map resolution the model was built for")
        self._resized.clear()  # parameters are about to change
        return self.engine.train_step(original_feats.reshape(b, h * w, c), denoised_feats.reshape(b, h * w, c),
                                      None if pred is None else pred.reshape(b, h * w, c))
