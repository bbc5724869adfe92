"""Reference for the tapped extractor forward (CPU, float64 by default): the residual stream after every asked block, all token
rows (prefix rows first), BEFORE the final LayerNorm.

It is the forward of tests/backbone_reference.py and tests/vitg_reference.py -- same operations in the same order, same
`round_bf16` comparator -- stopped after a block and without the final norm, over the union of their layouts: position table
with a cls row (DINOv2, DINO, AugReg), without one and without registers (DeiT-III), register tokens (reg4), GELU or packed
SwiGLU MLP, LayerScale keys or none.  tests/test_vit_taps_cpu.py pins it to those two files: `final_norm` of its rows is their
`forward_features(n_blocks=block + 1)`.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests import backbone_reference as bref


def residual_rows(sd: dict, img: torch.Tensor, patch: int, stride: int, blocks, eps: float = 1e-6,
                  dtype: torch.dtype = torch.float64, round_bf16: bool = False):
    """-> ({block: x [B, n_prefix + gh * gw, dim]}, (gh, gw, n_prefix)), x = the un-normed rows after that block."""
    dim = sd["pos_embed"].shape[-1]
    assert sd["patch_embed.proj.weight"].shape[-1] == patch
    heads = dim // 64
    n_reg = sd["reg_token"].shape[1] if "reg_token" in sd else 0
    r = (lambda t: t.to(torch.bfloat16).to(dtype)) if round_bf16 else (lambda t: t)  # a matrix operand
    W = lambda k: r(sd[k].to(dtype))  # noqa: E731  a weight matrix
    V = lambda k: sd[k].to(dtype)     # noqa: E731  a vector (fp32 in every mode)
    x = F.conv2d(r(img.to(dtype)), W("patch_embed.proj.weight"), V("patch_embed.proj.bias"), stride=stride)
    B, _, gh, gw = x.shape
    x = x.permute(0, 2, 3, 1).reshape(B, gh * gw, dim)
    has_cls = 0 if n_reg else bref.pos_has_cls(sd)
    pos = bref.resample_pos(sd["pos_embed"], (gh, gw), has_cls).to(dtype)  # (resampled in fp32, as the host does)
    cls = V("cls_token").expand(B, -1, -1)
    if n_reg:
        x = torch.cat([cls, V("reg_token").expand(B, -1, -1), x + pos], dim=1)
    elif has_cls:
        x = torch.cat([cls, x], dim=1) + pos
    else:
        x = torch.cat([cls, x + pos], dim=1)
    out = {}
    for i in range(max(blocks) + 1):
        p = f"blocks.{i}."
        h = r(F.layer_norm(x, (dim,), V(p + "norm1.weight"), V(p + "norm1.bias"), eps))
        qkv = r(F.linear(h, W(p + "attn.qkv.weight"), V(p + "attn.qkv.bias")))
        q, k, v = qkv.reshape(B, -1, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)
        a = r(r(torch.softmax((q * 0.125) @ k.transpose(-2, -1), dim=-1)) @ v)
        a = F.linear(a.transpose(1, 2).reshape(B, -1, dim), W(p + "attn.proj.weight"), V(p + "attn.proj.bias"))
        x = x + (V(p + "ls1.gamma") * a if p + "ls1.gamma" in sd else a)
        h = r(F.layer_norm(x, (dim,), V(p + "norm2.weight"), V(p + "norm2.bias"), eps))
        h = F.linear(h, W(p + "mlp.fc1.weight"), V(p + "mlp.fc1.bias"))
        if sd[p + "mlp.fc1.weight"].shape[0] == 2 * sd[p + "mlp.fc2.weight"].shape[1]:
            g, v = h.chunk(2, dim=-1)  # SwiGLUPacked: the gate is the FIRST half
            h = F.silu(g) * v
        else:
            h = F.gelu(h)
        h = F.linear(r(h), W(p + "mlp.fc2.weight"), V(p + "mlp.fc2.bias"))
        x = x + (V(p + "ls2.gamma") * h if p + "ls2.gamma" in sd else h)
        if i in blocks:
            out[i] = x
    return out, (gh, gw, 1 + n_reg)


def final_norm(sd: dict, x: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    dim = x.shape[-1]
    return F.layer_norm(x, (dim,), sd["norm.weight"].to(x.dtype), sd["norm.bias"].to(x.dtype), eps)
