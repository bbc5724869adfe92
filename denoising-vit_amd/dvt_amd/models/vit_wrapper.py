"""PretrainedViTWrapper on MI355X -- drop-in for dvt/models/vit_wrapper.py:59-146.

Same constructor arguments, properties (`n_output_dims`, `num_blocks`, `last_layer_index`,
`patch_size`, `stride`, `transformation`) and `get_intermediate_layers` signature; the timm
model behind it is replaced by the hand-written HIP forward (csrc/dvt_vit.hip and the GEMM / attention units it launches, csrc/dvt_vit_gemm.hip / dvt_vit_attn.hip).

Differences forced by the environment (documented in DESIGN.md):
  * no network / no timm: `pretrained=True` cannot download.  Weights come from
    `checkpoint_path=` (a timm-layout state dict saved with torch.save) or the environment
    variable DVT_VIT_CHECKPOINT.  Without either the constructor RAISES, like the reference
    does when the pretrained weights cannot be loaded -- features of a random ViT written to
    disk would be skipped forever by the existence-based resume.  Random init (seed 0) is
    available only on request (`allow_random_init=True`: synthetic benchmarks and tests).
  * the DINOv2 S/B/L/g backbones (with / without registers), the four DINO patch-8 / patch-16 models, DeiT-III B/16
    and AugReg B/16-384 are built (dvt_amd.vit.SPECS); the MAE, CLIP and EVA-02 ids of the reference's MODEL_LIST raise
    NotImplementedError with the reason (dvt_amd.vit.NOT_BUILT).  ViT-g/14
    (dim 1536, 40 blocks, SwiGLU MLP) runs in bfloat16 and exact float32; matmul="high" is refused.
  * the stride override (vit_wrapper.py:78-91) is honoured by the im2col kernel, but a
    grid other than the checkpoint's own is served by resampling pos_embed on the host (timm's
    resample_abs_pos_embed restated); the *_reg4_* models carry 4 register tokens (prefix tokens
    are stripped from the returned map like timm's `return_prefix_tokens=False`, and returned beside
    it, cls first, with `return_prefix_tokens=True`).
  * several `n` indices, `return_prefix_tokens` and `norm=False` come from ONE forward of the extractor
    (HipViT.forward_taps); `forward(x)` is the final-normed cls token.
"""
from __future__ import annotations

import os
import re
import warnings
from typing import List, Tuple, Union

import torch
import torch.nn as nn

from .. import vit as _vit

MODEL_LIST = [
    # DINOv1
    "vit_small_patch8_224.dino", "vit_small_patch16_224.dino", "vit_base_patch8_224.dino",
    "vit_base_patch16_224.dino",
    # DINOv2
    "vit_small_patch14_dinov2.lvd142m", "vit_base_patch14_dinov2.lvd142m",
    "vit_large_patch14_dinov2.lvd142m", "vit_giant_patch14_dinov2.lvd142m",
    # DINOv2 + register
    "vit_small_patch14_reg4_dinov2.lvd142m", "vit_base_patch14_reg4_dinov2.lvd142m",
    "vit_large_patch14_reg4_dinov2.lvd142m", "vit_giant_patch14_reg4_dinov2.lvd142m",
    # MAE
    "vit_base_patch16_224.mae", "vit_large_patch16_224.mae", "vit_huge_patch14_224.mae",
    # CLIP
    "vit_base_patch16_clip_384.laion2b_ft_in12k_in1k", "vit_base_patch16_clip_224.openai",
    # EVA
    "eva02_base_patch16_clip_224.merged2b",
    # DEiT-III
    "deit3_base_patch16_224.fb_in1k",
    # Auto-auged supervised ViT:
    "vit_base_patch16_384.augreg_in21k_ft_in1k",
]  # entry for entry the reference's list (dvt/models/vit_wrapper.py:15-56; its SAM / I-JEPA ids are commented out)

IMAGENET_MEAN, IMAGENET_STD = _vit.IMAGENET_MEAN, _vit.IMAGENET_STD


class Normalize:
    """Minimal stand-in for torchvision.transforms.Normalize (torchvision is absent here);
    the driver only reads `.mean` / `.std` (main_img_denoising.py:250-255)."""

    def __init__(self, mean, std):
        self.mean, self.std = tuple(mean), tuple(std)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        m = torch.as_tensor(self.mean, dtype=x.dtype, device=x.device).view(-1, 1, 1)
        s = torch.as_tensor(self.std, dtype=x.dtype, device=x.device).view(-1, 1, 1)
        return (x - m) / s


class Compose:
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class _PatchEmbedInfo:
    """Carries the attributes the reference touches on `model.patch_embed`."""

    class _Proj:
        def __init__(self, stride):
            self.stride = [stride, stride]

    def __init__(self, patch, stride):
        self.patch_size = (patch, patch)
        self.proj = self._Proj(stride)


class _ModelView(nn.Module):
    """`wrapper.model` of the reference exposes pos_embed / blocks / patch_embed; keep those."""

    def __init__(self, pos_embed, depth, patch, stride):
        super().__init__()
        self.register_buffer("pos_embed", pos_embed, persistent=False)
        self.blocks = nn.ModuleList([nn.Identity() for _ in range(depth)])
        self.patch_embed = _PatchEmbedInfo(patch, stride)


class PretrainedViTWrapper(nn.Module):
    def __init__(
        self,
        model_identifier: str = "vit_base_patch14_dinov2.lvd142m",
        stride: int = 7,
        dynamic_img_size: bool = True,
        dynamic_img_pad: bool = False,
        checkpoint_path: str | None = None,
        img_size: int | Tuple[int, int] | None = None,
        allow_random_init: bool = False,
        dtype: str = "bfloat16",
        **kwargs,
    ):
        super().__init__()
        assert model_identifier in MODEL_LIST, f"Model type {model_identifier} not tested yet."
        if model_identifier not in _vit.SPECS:
            why = _vit.NOT_BUILT.get(model_identifier)
            raise NotImplementedError(
                f"{model_identifier}: only {sorted(_vit.SPECS)} are built for MI355X (BASELINE.json)"
                + (f" -- {why}" if why else ""))
        self.model_identifier = model_identifier
        self.stride = stride
        self.patch_size = int(re.search(r"patch(\d+)", model_identifier).group(1))
        self.dynamic_img_size = dynamic_img_size
        self.dynamic_img_pad = dynamic_img_pad
        self.spec = _vit.SPECS[model_identifier]
        size = img_size or self.spec.img_size
        self.img_size = (size, size) if isinstance(size, int) else tuple(size)
        self.allow_random_init = bool(allow_random_init)
        # arithmetic of the extractor: "bfloat16" = the reference under autocast, "float32" = its default
        self.dtype = "float32" if str(dtype) in ("float32", "torch.float32", "fp32") else "bfloat16"
        self._state_dict, self.transformation = self.create_model(model_identifier, checkpoint_path)
        # a grid other than the checkpoint's (stride override vit_wrapper.py:78-91, other input
        # sizes) is handled by resampling pos_embed once on the host (dvt_amd.vit.resample_pos_embed)
        self.model = _ModelView(self._state_dict["pos_embed"].clone(), self.spec.depth,
                                self.patch_size, stride)
        self._hip = None

    def create_model(self, model_identifier: str, checkpoint_path: str | None = None):
        path = checkpoint_path or os.environ.get("DVT_VIT_CHECKPOINT")
        n_tokens = self.spec.n_pos  # rows of the position table: the checkpoint's grid, with or without a cls row
        if path:
            sd = torch.load(path, map_location="cpu")
            sd = sd.get("state_dict", sd.get("model", sd))
            # a stage-3 checkpoint holds the wrapper's state_dict: every key is `model.<timm key>`
            if sd and all(k.startswith("model.") for k in sd):
                sd = {k[len("model."):]: v for k, v in sd.items()}
        elif not self.allow_random_init:
            raise RuntimeError(
                f"{model_identifier}: no pretrained checkpoint (timm cannot download here). Pass "
                "checkpoint_path= / --vit_checkpoint or set DVT_VIT_CHECKPOINT to a timm-layout state "
                "dict; random weights need an explicit allow_random_init=True / --synthetic.")
        else:
            warnings.warn(f"{model_identifier}: RANDOM ViT weights (seed 0) on request -- synthetic "
                          "benchmarks and tests only")
            # O(1) LayerScale / biases / norm affines: with DINOv2's LayerScale init (1e-5) twelve
            # random blocks would be a numerical no-op and neither parity nor power draw would mean much
            sd = _vit.random_state_dict(self.spec.dim, self.spec.depth, self.spec.patch, n_tokens,
                                        seed=0, well_conditioned=True, n_reg=self.spec.n_reg, mlp=self.spec.mlp,
                                        layer_scale=self.spec.layer_scale)
        # timm data config of the model: ImageNet mean / std, 0.5 / 0.5 for AugReg
        return sd, Compose([Normalize(self.spec.mean, self.spec.std)])

    @property
    def n_output_dims(self) -> int:
        return self.model.pos_embed.shape[-1]

    @property
    def num_blocks(self) -> int:
        return len(self.model.blocks)

    @property
    def last_layer_index(self) -> int:
        return self.num_blocks - 1

    def _engine(self, device, dtype: str | None = None, matmul: str = "highest") -> "_vit.HipViT":
        dtype = dtype or self.dtype
        if not isinstance(self._hip, dict):
            self._hip = {}
        key = (torch.device(device), dtype, matmul)
        if key not in self._hip:
            self._hip[key] = _vit.HipViT(self._state_dict, self.patch_size, self.stride, self.img_size,
                                         device, dtype=dtype, matmul=matmul, pos_has_cls=self.spec.pos_has_cls)
        return self._hip[key]

    def features_nhwc(self, x: torch.Tensor, layer_index: int | None = None,
                      out: torch.Tensor | None = None, max_batch: int = 128,
                      dtype: str | None = None, matmul: str = "highest", return_cls: bool = False):
        """Fast path used by the stage-1 driver: NHWC fp32 patch-token map, optionally written
        straight into a slice of the feature store (no NCHW round trip).  `matmul` "high" (float32 only): linear
        layers through bf16x3 (dvt_amd.vit.HipViT).  return_cls: -> (map, cls [B, dim]), the final-normed cls token of the
        same forward (HipViT.forward_features)."""
        idx = self.last_layer_index if layer_index is None else layer_index
        return self._engine(x.device, dtype, matmul).forward_features(x.float(), n_blocks=idx + 1, out=out,
                                                                      max_batch=max_batch, return_cls=return_cls)

    def tap_indices(self, n: Union[int, List[int], Tuple[int]]) -> Tuple[List[int], List[int]]:
        """`n` of get_intermediate_layers -> (the block index of every returned entry, in the order of `n`; the unique
        ascending taps the one forward runs).  An int means the last n blocks; negative indices count from the end."""
        depth = self.num_blocks
        if isinstance(n, int):
            if not 1 <= n <= depth:
                raise ValueError(f"n={n}: a model of {depth} blocks has 1 to {depth} last blocks")
            order = list(range(depth - n, depth))
        else:
            order = [int(i) if int(i) >= 0 else depth + int(i) for i in n]
            if not order or any(i < 0 or i >= depth for i in order):
                raise ValueError(f"n={list(n)}: block indices of a model of {depth} blocks lie in [-{depth}, {depth})")
        return order, sorted(set(order))

    def get_intermediate_layers(
        self,
        x: torch.Tensor,
        n: Union[int, List[int], Tuple[int]] = 1,
        reshape: bool = True,
        return_prefix_tokens: bool = False,
        norm: bool = True,
    ) -> List[torch.Tensor]:
        """timm's `get_intermediate_layers` / `forward_intermediates` (vit_wrapper.py:122-143) from ONE forward of the HIP
        extractor: the blocks up to the highest index run once and every asked layer is tapped on the way
        (HipViT.forward_taps).  `n`: an int = the last n blocks, or block indices (negatives count from the end).  The results
        come back in the order of `n`, a repeated index as the same tensor; timm's own order for an unsorted list is not
        pinned here (timm is absent).  reshape=True: NCHW as a permuted view of the NHWC map, else [B, L, C].
        return_prefix_tokens=True: a list of (features, prefix_tokens [B, n_prefix, C]), all prefix rows: cls, then the
        registers.  norm=False: the rows before the final LayerNorm."""
        order, taps = self.tap_indices(n)
        eng = self._engine(x.device)
        res = {}
        step = _vit.DVT_VIT_MAX_TAPS  # (more layers than one call taps: the deeper groups start again from the patch embedding)
        for g in range(0, len(taps), step):
            got = eng.forward_taps(x.float(), taps[g:g + step], norm=norm, return_prefix=return_prefix_tokens)
            res.update(zip(taps[g:g + step], got))
        shaped = {}
        for i in taps:
            f, p = res[i] if return_prefix_tokens else (res[i], None)  # f: [B, gh, gw, C]
            # timm returns NCHW (`output_fmt="NCHW"`); a permuted view keeps the driver's
            # `.permute(0, 2, 3, 1)` (main_img_denoising.py:323) free
            f = f.permute(0, 3, 1, 2) if reshape else f.reshape(f.shape[0], -1, f.shape[-1])
            shaped[i] = (f, p) if return_prefix_tokens else f
        return [shaped[i] for i in order]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """The final-normed cls token [B, dim]: timm's forward_head(forward_features(x)) at num_classes=0 and
        global_pool="token", the configuration of all fourteen built ids -- restated from timm's source, not pinned against
        it (timm is absent)."""
        return self.features_nhwc(x, return_cls=True)[1]
