"""ViT-g/14 reference for the tests (CPU, float64 by default): the DINOv2 forward with the SwiGLU MLP.

Written from the published layout of timm 1.0.7's `vit_giant_patch14[_reg4]_dinov2` (timm is not installed):
  patch_embed (Conv2d dim x 3 x p x p, stride s) -> [cls, (reg), patches] + pos_embed (cls row only without registers)
  blocks:  x = x + ls1 * proj(softmax(q k^T / 8) v),  q, k, v = split(qkv(norm1(x)))        (head_dim 64)
           h = fc1(norm2(x)) [2 H];  g, v = h.chunk(2, -1);  x = x + ls2 * fc2(silu(g) * v)  (SwiGLUPacked, SiLU, no norm)
  -> norm(x) -> drop the prefix tokens -> [B, gh, gw, dim]   (LayerNorm eps 1e-6)
A state dict whose fc1 has as many rows as fc2 has columns takes the GELU MLP of the S / B / L models instead.

`round_bf16=True` is the comparator of the bf16 extractor's ARITHMETIC CLASS (the buffer list at the top of
csrc/dvt_vit.hip and its GEMM / attention units): every matrix operand (weights, LayerNorm outputs, q | k | v, the softmax probabilities, the attention
output, the hidden activations, the im2col patches) is rounded to bf16, everything else stays in `dtype`.

`to_hf_dinov2_swiglu`: the independent second opinion, transformers' Dinov2Model / Dinov2WithRegistersModel with
use_swiglu_ffn=True and the same weights (hidden width (int(dim * 4 * 2 / 3) + 7) // 8 * 8, weights_in chunked the same way).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def resample_pos(posemb: torch.Tensor, new_size, n_prefix_pos: int) -> torch.Tensor:
    """timm resample_abs_pos_embed: square source grid, bicubic + antialias in fp32, prefix rows carried over."""
    if new_size[0] * new_size[1] + n_prefix_pos == posemb.shape[1] and new_size[0] == new_size[1]:
        return posemb
    hw = int(math.sqrt(posemb.shape[1] - n_prefix_pos))
    prefix, grid = posemb[:, :n_prefix_pos], posemb[:, n_prefix_pos:]
    dim = posemb.shape[-1]
    grid = grid.float().reshape(1, hw, hw, dim).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=tuple(new_size), mode="bicubic", antialias=True)
    return torch.cat([prefix, grid.permute(0, 2, 3, 1).reshape(1, -1, dim).to(posemb.dtype)], dim=1)


def forward_features(sd: dict, img: torch.Tensor, patch: int, stride: int, n_blocks: int | None = None, eps: float = 1e-6,
                     dtype: torch.dtype = torch.float64, return_cls: bool = False, round_bf16: bool = False):
    dim = sd["pos_embed"].shape[-1]
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    n_blocks = depth if n_blocks is None else n_blocks
    heads = dim // 64
    n_reg = sd["reg_token"].shape[1] if "reg_token" in sd else 0
    r = (lambda t: t.to(torch.bfloat16).to(dtype)) if round_bf16 else (lambda t: t)  # a matrix operand
    W = lambda k: r(sd[k].to(dtype))  # noqa: E731  a weight matrix
    V = lambda k: sd[k].to(dtype)     # noqa: E731  a vector (fp32 in every mode)
    x = F.conv2d(r(img.to(dtype)), W("patch_embed.proj.weight"), V("patch_embed.proj.bias"), stride=stride)
    B, _, gh, gw = x.shape
    x = x.permute(0, 2, 3, 1).reshape(B, gh * gw, dim)
    pos = resample_pos(sd["pos_embed"], (gh, gw), 0 if n_reg else 1).to(dtype)  # (resampled in fp32, as the host does)
    cls = V("cls_token").expand(B, -1, -1)
    if n_reg:
        x = torch.cat([cls, V("reg_token").expand(B, -1, -1), x + pos], dim=1)
    else:
        x = torch.cat([cls, x], dim=1) + pos
    for i in range(n_blocks):
        p = f"blocks.{i}."
        h = r(F.layer_norm(x, (dim,), V(p + "norm1.weight"), V(p + "norm1.bias"), eps))
        qkv = r(F.linear(h, W(p + "attn.qkv.weight"), V(p + "attn.qkv.bias")))
        q, k, v = qkv.reshape(B, -1, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)
        a = r(r(torch.softmax((q * 0.125) @ k.transpose(-2, -1), dim=-1)) @ v)
        a = F.linear(a.transpose(1, 2).reshape(B, -1, dim), W(p + "attn.proj.weight"), V(p + "attn.proj.bias"))
        x = x + V(p + "ls1.gamma") * a
        h = r(F.layer_norm(x, (dim,), V(p + "norm2.weight"), V(p + "norm2.bias"), eps))
        h = F.linear(h, W(p + "mlp.fc1.weight"), V(p + "mlp.fc1.bias"))
        if sd[p + "mlp.fc1.weight"].shape[0] == 2 * sd[p + "mlp.fc2.weight"].shape[1]:
            g, v = h.chunk(2, dim=-1)  # SwiGLUPacked: the gate is the FIRST half
            h = F.silu(g) * v
        else:
            h = F.gelu(h)
        x = x + V(p + "ls2.gamma") * F.linear(r(h), W(p + "mlp.fc2.weight"), V(p + "mlp.fc2.bias"))
    x = F.layer_norm(x, (dim,), V("norm.weight"), V("norm.bias"), eps)
    feat = x[:, 1 + n_reg:].reshape(B, gh, gw, dim)
    return (feat, x[:, 0]) if return_cls else feat


def to_hf_dinov2_swiglu(sd: dict, img_size: int, patch: int):
    """transformers Dinov2Model (Dinov2WithRegistersModel when `reg_token` is there) with use_swiglu_ffn=True carrying the
    weights of a timm-layout SwiGLU state dict.  HF's register model keeps a cls row in its position table: set to zero."""
    dim = sd["pos_embed"].shape[-1]
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    n_reg = sd["reg_token"].shape[1] if "reg_token" in sd else 0
    kw = dict(hidden_size=dim, num_hidden_layers=depth, num_attention_heads=dim // 64, mlp_ratio=4, image_size=img_size,
              patch_size=patch, layer_norm_eps=1e-6, qkv_bias=True, layerscale_value=1.0, use_swiglu_ffn=True,
              attn_implementation="eager")
    hf = {}
    if n_reg:
        from transformers import Dinov2WithRegistersConfig, Dinov2WithRegistersModel
        m = Dinov2WithRegistersModel(Dinov2WithRegistersConfig(num_register_tokens=n_reg, **kw)).eval()
        hf["embeddings.register_tokens"] = sd["reg_token"]
        pos = torch.cat([torch.zeros(1, 1, dim), sd["pos_embed"]], dim=1)
    else:
        from transformers import Dinov2Config, Dinov2Model
        m = Dinov2Model(Dinov2Config(**kw)).eval()
        pos = sd["pos_embed"]
    hf["embeddings.cls_token"] = sd["cls_token"]
    hf["embeddings.position_embeddings"] = pos
    hf["embeddings.patch_embeddings.projection.weight"] = sd["patch_embed.proj.weight"]
    hf["embeddings.patch_embeddings.projection.bias"] = sd["patch_embed.proj.bias"]
    for i in range(depth):
        p, q = f"blocks.{i}.", f"encoder.layer.{i}."
        wq, wk, wv = sd[p + "attn.qkv.weight"].chunk(3, 0)
        bq, bk, bv = sd[p + "attn.qkv.bias"].chunk(3, 0)
        for nm, w_, b_ in (("query", wq, bq), ("key", wk, bk), ("value", wv, bv)):
            hf[q + f"attention.attention.{nm}.weight"] = w_
            hf[q + f"attention.attention.{nm}.bias"] = b_
        hf[q + "attention.output.dense.weight"] = sd[p + "attn.proj.weight"]
        hf[q + "attention.output.dense.bias"] = sd[p + "attn.proj.bias"]
        for nm in ("norm1", "norm2"):
            hf[q + nm + ".weight"], hf[q + nm + ".bias"] = sd[p + nm + ".weight"], sd[p + nm + ".bias"]
        hf[q + "layer_scale1.lambda1"] = sd[p + "ls1.gamma"]
        hf[q + "layer_scale2.lambda1"] = sd[p + "ls2.gamma"]
        hf[q + "mlp.weights_in.weight"], hf[q + "mlp.weights_in.bias"] = sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]
        hf[q + "mlp.weights_out.weight"], hf[q + "mlp.weights_out.bias"] = sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"]
    hf["layernorm.weight"], hf["layernorm.bias"] = sd["norm.weight"], sd["norm.bias"]
    missing, unexpected = m.load_state_dict(hf, strict=False)
    assert not unexpected, unexpected
    assert all("mask_token" in k for k in missing), missing
    return m
