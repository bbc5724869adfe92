"""Host side of the stage-2 denoiser's bf16 inference forward (csrc/dvt_denoiser.hip, C ABI in include/dvt_denoiser.h).

`HipDenoiser` holds one parameter version of a `Stage2Engine` at one token grid in the form the extractor's block kernels
read: bf16 matrices, the LayerNorm-folded matrices with their column sums and biases (dim 768 / 1024; dim 384 runs the
LayerNorm kernels), fp32 vectors, LayerScale ones (the reference's Block has none) and the position table resampled to the
grid.  Two forwards: `forward` (features in) and `forward_fused` (image in, through a bf16 `HipViT`, one launch sequence).
Opt-in (`Denoiser(inference_dtype="bfloat16")`); the exact-fp32 forward of the trainer stays `Stage2Engine.forward`.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib, s2
from .vit import HipViT, VitBlockWeights, VitConfig, VitWeights, fold_layernorm, resample_pos_embed

MAX_BLOCKS = s2.MAX_BLOCKS  # == DVT_DENOISER_MAX_BLOCKS (the struct layout check below would notice)


class DenoiserConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dim", "heads", "mlp_dim", "n_blocks", "grid_h", "grid_w", "n_tokens", "s_pad",
                                         "enable_pe")] + [("ln_eps", C.c_float)]


class DenoiserWeights(C.Structure):
    _fields_ = [("pos_embed", C.c_void_p), ("blocks", VitBlockWeights * MAX_BLOCKS)]


_P, _I = C.c_void_p, C.c_int
_lib.register_signatures({
    "dvt_denoiser_config": (_I, [_I, _I, _I, _I, _I, _I, C.POINTER(DenoiserConfig)]),
    "dvt_denoiser_struct_sizes": (_I, [C.POINTER(C.c_int64)]),
    "dvt_denoiser_workspace_bytes": (C.c_int64, [C.POINTER(DenoiserConfig), _I]),
    "dvt_denoiser_forward_bf16": (_I, [C.POINTER(DenoiserConfig), C.POINTER(DenoiserWeights), _P, _P, _I, _P, _P]),
    "dvt_vit_workspace_bytes_denoised": (C.c_int64, [C.POINTER(VitConfig), C.POINTER(DenoiserConfig), _I]),
    "dvt_vit_forward_denoised": (_I, [C.POINTER(VitConfig), C.POINTER(VitWeights), C.POINTER(DenoiserConfig),
                                      C.POINTER(DenoiserWeights), _P, _P, _P, _P, _I, _P, _P]),
})


def row_pad() -> int:
    """Rows an image's tokens are padded to: 32, or DVT_VIT_ROW_PAD (the extractor's knob, HipViT)."""
    env = os.environ.get("DVT_VIT_ROW_PAD", "")
    return int(env) if env.isdigit() and int(env) > 0 else 32


def denoiser_config(dim: int, n_blocks: int, grid: tuple[int, int], enable_pe: bool, pad: int | None = None) -> DenoiserConfig:
    cfg = DenoiserConfig()
    _lib.check(_lib.lib().dvt_denoiser_config(dim, n_blocks, grid[0], grid[1], int(bool(enable_pe)),
                                              row_pad() if pad is None else pad, C.byref(cfg)), "dvt_denoiser_config")
    sizes = (C.c_int64 * 2)()
    _lib.lib().dvt_denoiser_struct_sizes(sizes)
    if list(sizes) != [C.sizeof(DenoiserConfig), C.sizeof(DenoiserWeights)]:
        raise _lib.DvtError("denoiser struct layout mismatch between ctypes and C")
    return cfg


class HipDenoiser:
    """Device-resident bf16 weights of a denoiser at one grid + the two forward launchers."""

    def __init__(self, state: dict, noise_map_size: tuple[int, int], grid: tuple[int, int], num_blocks: int = 1,
                 enable_pe: bool = True, device: torch.device | str = "cuda"):
        """`state`: the Denoiser's state-dict names (`pos_embed`, `denoiser.<tensor>`, `denoiser.<i>.<tensor>` for
        num_blocks > 1) -> fp32 tensors, e.g. `Stage2Engine.views()`; `noise_map_size` is the grid of its pos_embed."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DvtError("HipDenoiser needs a HIP device; there is no CPU fallback")
        key0 = "denoiser.norm1.weight" if num_blocks == 1 else "denoiser.0.norm1.weight"
        dim = int(state[key0].shape[0])
        s2.make_config(dim, grid[0] * grid[1], num_blocks, enable_pe)  # the widths / block counts stage 2 is built for
        self.cfg = denoiser_config(dim, num_blocks, grid, enable_pe)
        self.grid = tuple(grid)
        self._keep = []
        sd = {k: v.detach().to("cpu", torch.float32) for k, v in state.items()}

        def f32(t):
            t = t.to(self.device, torch.float32).contiguous()
            self._keep.append(t)
            return t.data_ptr()

        def bf16(t):
            t = t.to(self.device, torch.bfloat16).contiguous()
            self._keep.append(t)
            return t.data_ptr()

        w = DenoiserWeights()
        if enable_pe:
            gh, gw = noise_map_size
            pos = sd["pos_embed"].reshape(1, gh * gw, dim)
            if (gh, gw) != self.grid:  # (the table's own grid need not be square; a resampled one's source must be)
                pos = resample_pos_embed(pos, self.grid, 0)
            w.pos_embed = f32(pos.reshape(grid[0] * grid[1], dim))
        ones = f32(torch.ones(dim))  # no LayerScale in the reference's Block
        for i in range(num_blocks):
            p, b = ("denoiser." if num_blocks == 1 else f"denoiser.{i}."), w.blocks[i]
            b.norm1_w, b.norm1_b = f32(sd[p + "norm1.weight"]), f32(sd[p + "norm1.bias"])
            b.qkv_w, b.qkv_b = bf16(sd[p + "attn.qkv.weight"]), f32(sd[p + "attn.qkv.bias"])
            b.proj_w, b.proj_b = bf16(sd[p + "attn.proj.weight"]), f32(sd[p + "attn.proj.bias"])
            b.norm2_w, b.norm2_b = f32(sd[p + "norm2.weight"]), f32(sd[p + "norm2.bias"])
            b.fc1_w, b.fc1_b = bf16(sd[p + "mlp.fc1.weight"]), f32(sd[p + "mlp.fc1.bias"])
            b.fc2_w, b.fc2_b = bf16(sd[p + "mlp.fc2.weight"]), f32(sd[p + "mlp.fc2.bias"])
            b.ls1 = b.ls2 = ones
            if dim % 256 == 0:  # the folded path's shapes (include/dvt_denoiser.h); dim 384 runs the LayerNorm kernels
                for norm, lin, dst in (("norm1", "attn.qkv", "qkv"), ("norm2", "mlp.fc1", "fc1")):
                    Wf, cs, bf = fold_layernorm(sd[p + lin + ".weight"], sd[p + lin + ".bias"], sd[p + norm + ".weight"],
                                                sd[p + norm + ".bias"])
                    setattr(b, dst + "_wf", bf16(Wf))
                    setattr(b, dst + "_cs", f32(cs))
                    setattr(b, dst + "_bf", f32(bf))
        self.weights = w
        self._ws = {}  # "alone" / the fused extractor's config bytes -> (batch, buffer), grow-only

    def _workspace(self, key, batch: int, size_fn) -> torch.Tensor:
        have = self._ws.get(key)
        if have is None or have[0] < batch:
            n = int(size_fn(batch))
            if n <= 0:
                raise _lib.DvtError("denoiser workspace: invalid configuration")
            have = (batch, torch.empty(n, device=self.device, dtype=torch.uint8))
            self._ws[key] = have
        return have[1]

    def forward(self, feats: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """feats [B, gh, gw, dim] (or [B, gh * gw, dim]) fp32 -> blocks(feats + pos_embed), same shape (dvt_denoiser_forward_bf16)."""
        _lib.require_cuda(feats, out)
        cfg = self.cfg
        if feats.dtype != torch.float32 or feats.shape[-1] != cfg.dim or feats.shape[1:].numel() != cfg.n_tokens * cfg.dim:
            raise _lib.DvtError(f"expected fp32 [B, {cfg.grid_h}, {cfg.grid_w}, {cfg.dim}], got {tuple(feats.shape)} {feats.dtype}")
        feats = feats.contiguous()
        out = torch.empty_like(feats) if out is None else out
        if out.dtype != torch.float32 or not out.is_contiguous() or out.shape != feats.shape:
            raise _lib.DvtError("out must be a contiguous fp32 tensor of the input's shape")
        B = feats.shape[0]
        L = _lib.lib()
        ws = self._workspace("alone", B, lambda b: L.dvt_denoiser_workspace_bytes(C.byref(cfg), b))
        _lib.check(L.dvt_denoiser_forward_bf16(C.byref(cfg), C.byref(self.weights), feats.data_ptr(), out.data_ptr(), B,
                                               ws.data_ptr(), _lib.stream()), "dvt_denoiser_forward_bf16")
        return out

    def forward_fused(self, vit: HipViT, img: torch.Tensor, return_original: bool = False, return_cls: bool = False,
                      max_batch: int = 128):
        """img [B, 3, H, W] fp32 (normalised) -> (denoised [B, gh, gw, dim], original_feats or None, cls [B, dim] or None)
        from one launch sequence per launch of the extractor's plan (dvt_vit_forward_denoised): `original_feats` holds the
        bits of vit.forward_features, `cls` those of its return_cls form, `denoised` those of forward(original_feats)."""
        _lib.require_cuda(img)
        vc, cfg = vit.cfg, self.cfg
        if vit.dtype != "bfloat16" or vit.x3:
            raise _lib.DvtError("the fused denoiser forward runs on a bfloat16 HipViT")
        if img.dtype != torch.float32 or tuple(img.shape[1:]) != (3, vc.img_h, vc.img_w):
            raise _lib.DvtError(f"expected fp32 [B,3,{vc.img_h},{vc.img_w}], got {tuple(img.shape)} {img.dtype}")
        if (vc.grid_h, vc.grid_w, vc.dim) != (cfg.grid_h, cfg.grid_w, cfg.dim):
            raise _lib.DvtError(f"the extractor's {vc.grid_h}x{vc.grid_w}x{vc.dim} tokens are not the denoiser's "
                                f"{cfg.grid_h}x{cfg.grid_w}x{cfg.dim}")
        img = img.contiguous()
        B = img.shape[0]
        shape = (B, cfg.grid_h, cfg.grid_w, cfg.dim)
        new = lambda *s: torch.empty(s, device=self.device, dtype=torch.float32)  # noqa: E731
        out, orig, cls = new(*shape), new(*shape) if return_original else None, new(B, cfg.dim) if return_cls else None
        plan = vit.launch_plan(B, max_batch)
        L = _lib.lib()
        ws = self._workspace(bytes(vc), max(plan), lambda b: L.dvt_vit_workspace_bytes_denoised(C.byref(vc), C.byref(cfg), b))
        b0 = 0
        for nb in plan:
            _lib.check(L.dvt_vit_forward_denoised(C.byref(vc), C.byref(vit.weights), C.byref(cfg), C.byref(self.weights),
                                                  img[b0:].data_ptr(), out[b0:].data_ptr(),
                                                  orig[b0:].data_ptr() if return_original else None,
                                                  cls[b0:].data_ptr() if return_cls else None, nb, ws.data_ptr(),
                                                  _lib.stream()), "dvt_vit_forward_denoised")
            b0 += nb
        return out, orig, cls
