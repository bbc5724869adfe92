"""Reference for the stage-2 `Denoiser`'s forward on features (CPU, float64 by default).

Restated from the reference's dvt/models/online_denoiser.py:59-104 and timm's Block:
  x = feats [B, gh * gw, dim] + pos_embed           (enable_pe; another grid: the table resampled bicubic + antialias in fp32)
  num_blocks x:  x = x + proj(softmax(q k^T / 8) v),  q, k, v = split(qkv(norm1(x)))   (head_dim 64, LayerNorm eps 1e-6)
                 x = x + fc2(gelu(fc1(norm2(x))))                                       (exact GELU; no LayerScale)
  no final norm.
State-dict names are the Denoiser's: `pos_embed`, `denoiser.<tensor>` (`denoiser.<i>.<tensor>` for num_blocks > 1).

`round_bf16=True` is the comparator of the bf16 forward's arithmetic class, as in tests/backbone_reference.py: every matrix
operand is rounded to bf16, everything else stays in `dtype`.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests.backbone_reference import resample_pos

BLOCK_TENSORS = ["norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                 "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"]


def block_prefix(i: int, num_blocks: int) -> str:
    return "denoiser." if num_blocks == 1 else f"denoiser.{i}."


def random_denoiser_state(dim: int, num_blocks: int, noise_map: tuple[int, int], seed: int = 0, enable_pe: bool = True) -> dict:
    """Well-conditioned random weights under the Denoiser's names: the block keys of dvt_amd.vit.random_state_dict (O(1) biases
    and norm affines, no LayerScale) and a pos_embed of scale 0.02."""
    from dvt_amd.vit import random_state_dict
    src = random_state_dict(dim, num_blocks, 14, 1, seed=seed, well_conditioned=True, layer_scale=False)
    sd = {}
    if enable_pe:
        g = torch.Generator().manual_seed(seed + 1000)
        sd["pos_embed"] = torch.randn(1, noise_map[0] * noise_map[1], dim, generator=g) * 0.02
    for i in range(num_blocks):
        for t in BLOCK_TENSORS:
            sd[block_prefix(i, num_blocks) + t] = src[f"blocks.{i}.{t}"]
    return sd


def layernorm_like_features(batch: int, grid: tuple[int, int], dim: int, seed: int = 0) -> torch.Tensor:
    """What a final LayerNorm hands the denoiser: rows of unit variance plus a per-channel offset of order 1 (fp32, NHWC)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, grid[0], grid[1], dim, generator=g)
    x = (x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True)
    return (x + torch.randn(dim, generator=g)).float()


def forward(sd: dict, feats: torch.Tensor, num_blocks: int = 1, noise_map: tuple[int, int] | None = None, eps: float = 1e-6,
            dtype: torch.dtype = torch.float64, round_bf16: bool = False) -> torch.Tensor:
    """feats [B, gh, gw, dim] -> the denoised features, same shape.  `pos_embed` (where the state has one) belongs to the
    `noise_map` grid (default: the features' own) and is resampled to the features' grid."""
    B, gh, gw, dim = feats.shape
    heads = dim // 64
    r = (lambda t: t.to(torch.bfloat16).to(dtype)) if round_bf16 else (lambda t: t)  # a matrix operand
    x = feats.to(dtype).reshape(B, gh * gw, dim)
    if "pos_embed" in sd:
        pos = sd["pos_embed"]
        if noise_map is not None and tuple(noise_map) != (gh, gw):
            pos = resample_pos(pos, (gh, gw), 0)  # (in fp32, as the host does)
        assert pos.shape[1] == gh * gw
        x = x + pos.to(dtype)
    for i in range(num_blocks):
        p = block_prefix(i, num_blocks)
        W = lambda k: r(sd[p + k].to(dtype))  # noqa: E731  a weight matrix
        V = lambda k: sd[p + k].to(dtype)     # noqa: E731  a vector (fp32 in every mode)
        h = r(F.layer_norm(x, (dim,), V("norm1.weight"), V("norm1.bias"), eps))
        qkv = r(F.linear(h, W("attn.qkv.weight"), V("attn.qkv.bias")))
        q, k, v = qkv.reshape(B, -1, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)
        a = r(r(torch.softmax((q * 0.125) @ k.transpose(-2, -1), dim=-1)) @ v)
        x = x + F.linear(a.transpose(1, 2).reshape(B, -1, dim), W("attn.proj.weight"), V("attn.proj.bias"))
        h = r(F.layer_norm(x, (dim,), V("norm2.weight"), V("norm2.bias"), eps))
        h = r(F.gelu(F.linear(h, W("mlp.fc1.weight"), V("mlp.fc1.bias"))))
        x = x + F.linear(h, W("mlp.fc2.weight"), V("mlp.fc2.bias"))
    return x.reshape(B, gh, gw, dim)
