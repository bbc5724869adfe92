"""Reference for the DINO / DeiT-III / AugReg patch-8 / patch-16 backbones (CPU, float64 by default).

Written from the published architectures (timm 1.0.7's `vit_{small,base}_patch{8,16}_224.dino`, `deit3_base_patch16_224`,
`vit_base_patch16_384.augreg_in21k_ft_in1k`; timm is not installed, parity with it is unpinned):
  patch_embed (Conv2d dim x 3 x p x p, stride s) -> tokens
  position table WITH a cls row (DINO, AugReg; timm no_embed_class=False):  x = cat(cls, patches) + pos
  position table WITHOUT one (DeiT-III; timm no_embed_class=True):           x = cat(cls, patches + pos)
  (another grid: the patch rows of the table resampled bicubic + antialias in fp32, the cls row carried over)
  blocks:  x = x + ls1 * proj(softmax(q k^T / 8) v),  q, k, v = split(qkv(norm1(x)))   (head_dim 64, LayerNorm eps 1e-6)
           x = x + ls2 * fc2(gelu(fc1(norm2(x))))                                       (exact GELU)
           ls1 / ls2 = 1 where the state dict has no `ls*.gamma` keys (DINO, AugReg)
  -> norm(x) -> drop the cls token -> [B, gh, gw, dim]
Whether the table has a cls row is read from its row count (a square: none; a square plus one: cls first) unless given.

`round_bf16=True` is the comparator of the bf16 extractor's arithmetic class, as in tests/vitg_reference.py: every matrix
operand is rounded to bf16, everything else stays in `dtype`.

`to_hf_vit`: the independent second opinion, transformers.ViTModel (layer_norm_eps 1e-6, no pooler) with the same weights;
it fits the cls + patches layout without LayerScale.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def pos_has_cls(sd: dict) -> int:
    n = int(sd["pos_embed"].shape[1])
    return 0 if math.isqrt(n) ** 2 == n else 1


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


def embed(sd: dict, img: torch.Tensor, stride: int, dtype=torch.float64, round_bf16: bool = False, has_cls: int | None = None):
    """The input of block 0: [B, 1 + gh * gw, dim], and the grid."""
    dim = sd["pos_embed"].shape[-1]
    r = (lambda t: t.to(torch.bfloat16).to(dtype)) if round_bf16 else (lambda t: t)
    x = F.conv2d(r(img.to(dtype)), r(sd["patch_embed.proj.weight"].to(dtype)), sd["patch_embed.proj.bias"].to(dtype),
                 stride=stride)
    B, _, gh, gw = x.shape
    x = x.permute(0, 2, 3, 1).reshape(B, gh * gw, dim)
    has_cls = pos_has_cls(sd) if has_cls is None else int(has_cls)
    pos = resample_pos(sd["pos_embed"], (gh, gw), has_cls).to(dtype)  # (resampled in fp32, as the host does)
    cls = sd["cls_token"].to(dtype).expand(B, -1, -1)
    x = torch.cat([cls, x], dim=1) + pos if has_cls else torch.cat([cls, x + pos], dim=1)
    return x, gh, gw


def forward_features(sd: dict, img: torch.Tensor, patch: int, stride: int, n_blocks: int | None = None, eps: float = 1e-6,
                     dtype: torch.dtype = torch.float64, return_cls: bool = False, round_bf16: bool = False,
                     has_cls: int | None = None):
    dim = sd["pos_embed"].shape[-1]
    assert sd["patch_embed.proj.weight"].shape[-1] == patch and "reg_token" not in sd
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    n_blocks = depth if n_blocks is None else n_blocks
    heads = dim // 64
    r = (lambda t: t.to(torch.bfloat16).to(dtype)) if round_bf16 else (lambda t: t)  # a matrix operand
    W = lambda k: r(sd[k].to(dtype))  # noqa: E731  a weight matrix
    V = lambda k: sd[k].to(dtype)     # noqa: E731  a vector (fp32 in every mode)
    x, gh, gw = embed(sd, img, stride, dtype, round_bf16, has_cls)
    B = x.shape[0]
    for i in range(n_blocks):
        p = f"blocks.{i}."
        h = r(F.layer_norm(x, (dim,), V(p + "norm1.weight"), V(p + "norm1.bias"), eps))
        qkv = r(F.linear(h, W(p + "attn.qkv.weight"), V(p + "attn.qkv.bias")))
        q, k, v = qkv.reshape(B, -1, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)
        a = r(r(torch.softmax((q * 0.125) @ k.transpose(-2, -1), dim=-1)) @ v)
        a = F.linear(a.transpose(1, 2).reshape(B, -1, dim), W(p + "attn.proj.weight"), V(p + "attn.proj.bias"))
        x = x + (V(p + "ls1.gamma") * a if p + "ls1.gamma" in sd else a)
        h = r(F.layer_norm(x, (dim,), V(p + "norm2.weight"), V(p + "norm2.bias"), eps))
        h = r(F.gelu(F.linear(h, W(p + "mlp.fc1.weight"), V(p + "mlp.fc1.bias"))))
        h = F.linear(h, W(p + "mlp.fc2.weight"), V(p + "mlp.fc2.bias"))
        x = x + (V(p + "ls2.gamma") * h if p + "ls2.gamma" in sd else h)
    x = F.layer_norm(x, (dim,), V("norm.weight"), V("norm.bias"), eps)
    feat = x[:, 1:].reshape(B, gh, gw, dim)
    return (feat, x[:, 0]) if return_cls else feat


def to_hf_vit(sd: dict, img_size: int, patch: int):
    """transformers.ViTModel carrying a timm-layout state dict with a cls + patches position table and no LayerScale.
    Two generations of parameter names are known (`encoder.layer.N.attention.attention.query` and `layers.N.attention.q_proj`);
    the one the installed class uses is read from its own state dict."""
    from transformers import ViTConfig, ViTModel
    dim = sd["pos_embed"].shape[-1]
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    assert "blocks.0.ls1.gamma" not in sd and pos_has_cls(sd) == 1
    cfg = ViTConfig(hidden_size=dim, num_hidden_layers=depth, num_attention_heads=dim // 64, intermediate_size=4 * dim,
                    image_size=img_size, patch_size=patch, layer_norm_eps=1e-6, hidden_act="gelu", qkv_bias=True,
                    hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, attn_implementation="eager")
    m = ViTModel(cfg, add_pooling_layer=False).eval()
    names = set(m.state_dict())
    new = "layers.0.attention.q_proj.weight" in names
    hf = {"embeddings.cls_token": sd["cls_token"], "embeddings.position_embeddings": sd["pos_embed"],
          "embeddings.patch_embeddings.projection.weight": sd["patch_embed.proj.weight"],
          "embeddings.patch_embeddings.projection.bias": sd["patch_embed.proj.bias"],
          "layernorm.weight": sd["norm.weight"], "layernorm.bias": sd["norm.bias"]}
    for i in range(depth):
        p = f"blocks.{i}."
        q = f"layers.{i}." if new else f"encoder.layer.{i}."
        wq, wk, wv = sd[p + "attn.qkv.weight"].chunk(3, 0)
        bq, bk, bv = sd[p + "attn.qkv.bias"].chunk(3, 0)
        qkv_names = ("attention.q_proj", "attention.k_proj", "attention.v_proj") if new else \
            ("attention.attention.query", "attention.attention.key", "attention.attention.value")
        for nm, w_, b_ in zip(qkv_names, (wq, wk, wv), (bq, bk, bv)):
            hf[q + nm + ".weight"], hf[q + nm + ".bias"] = w_, b_
        o = "attention.o_proj" if new else "attention.output.dense"
        hf[q + o + ".weight"], hf[q + o + ".bias"] = sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"]
        f1, f2 = ("mlp.fc1", "mlp.fc2") if new else ("intermediate.dense", "output.dense")
        for src, dst in (("norm1", "layernorm_before"), ("norm2", "layernorm_after"), ("mlp.fc1", f1), ("mlp.fc2", f2)):
            hf[q + dst + ".weight"], hf[q + dst + ".bias"] = sd[p + src + ".weight"], sd[p + src + ".bias"]
    assert set(hf) == names, sorted(set(hf) ^ names)[:8]
    m.load_state_dict(hf, strict=True)
    return m
