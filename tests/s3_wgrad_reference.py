"""Comparator of the stage-3 step's bf16 weight gradients (tests helper, CPU; include/dvt_stage3.h gemm_modes 5 and 7,
csrc/dvt_s3_wgrad.hip): the float64 step of tests/s3_reference.py in which each of a block's four linear layers rounds what the
modes round and nothing else --

    forward         y  = bf16(x)  . bf16(W)^T + b           as tests/s3_bf16_reference.py `MixedLinear`
    data gradient   dx = bf16(dy) . bf16(W)                 as `MixedLinear`
    weight gradient dW = bf16(dy)^T . bf16(x)               the modes' addition
    bias gradient   db = colsum(dy)                         from the UNROUNDED dy

-- with every product exact (float64).  `attention=False` is gemm_mode 5: the plain float64 attention between those layers;
`attention=True` is gemm_mode 7: `FlashAttention` and `qkv_bias` of tests/s3_attn_reference.py.  `rounding=False` switches every
rounding off: plain float64 autograd, which tests/test_stage3_wgrad_cpu.py holds to tests/s3_reference.py."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import vit as OV
from tests import s3_attn_reference as ATT
from tests import s3_bf16_reference as MP
from tests import s3_reference as REF


class WgradLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, rounding):
        ctx.save_for_backward(x, w)
        ctx.rounding = rounding
        r = MP.bf16 if rounding else (lambda t: t)
        return r(x) @ r(w).t() + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        r = MP.bf16 if ctx.rounding else (lambda t: t)
        dyb = r(dy)
        dy2, dyb2, x2 = dy.reshape(-1, dy.shape[-1]), dyb.reshape(-1, dy.shape[-1]), r(x).reshape(-1, x.shape[-1])
        return dyb @ r(w), dyb2.t() @ x2, dy2.sum(0), None


def forward_features(sd: dict, img: torch.Tensor, patch: int, stride: int, rounding: bool = True, attention: bool = False,
                     eps: float = 1e-6):
    """tests/s3_bf16_reference.py `forward_features` with the four linear layers of a block as WgradLinear, and with
    `attention` the attention and the qkv bias of tests/s3_attn_reference.py."""
    dim = sd["pos_embed"].shape[-1]
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    heads = dim // 64
    lin = lambda h, name: WgradLinear.apply(h, sd[name + ".weight"], sd[name + ".bias"], rounding)  # noqa: E731
    x = F.conv2d(img, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=stride)
    B, _, gh, gw = x.shape
    x = x.permute(0, 2, 3, 1).reshape(B, gh * gw, dim)
    n_reg = sd["reg_token"].shape[1] if "reg_token" in sd else 0
    pos = OV.resample_abs_pos_embed(sd["pos_embed"], (gh, gw), num_prefix_tokens=0 if n_reg else 1)
    if n_reg:
        x = torch.cat([sd["cls_token"].expand(B, -1, -1), sd["reg_token"].expand(B, -1, -1), x + pos], dim=1)
    else:
        x = torch.cat([sd["cls_token"].expand(B, -1, -1), x], dim=1) + pos
    for i in range(depth):
        p = f"blocks.{i}."
        h = F.layer_norm(x, (dim,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
        qb = sd[p + "attn.qkv.bias"]
        qkv = WgradLinear.apply(h, sd[p + "attn.qkv.weight"], ATT.qkv_bias(qb, rounding) if attention else qb, rounding)
        q, k, v = qkv.reshape(B, -1, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)
        if attention:
            a = ATT.attention(q, k, v, rounding)
        else:
            a = torch.softmax((q * 64 ** -0.5) @ k.transpose(-2, -1), dim=-1) @ v
        a = lin(a.transpose(1, 2).reshape(B, -1, dim), p + "attn.proj")
        x = x + sd[p + "ls1.gamma"] * a
        h = F.layer_norm(x, (dim,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
        h = lin(F.gelu(lin(h, p + "mlp.fc1")), p + "mlp.fc2")
        x = x + sd[p + "ls2.gamma"] * h
    x = F.layer_norm(x, (dim,), sd["norm.weight"], sd["norm.bias"], eps)
    return x[:, 1 + n_reg:].reshape(B, gh, gw, dim)


def step(sd: dict, img: torch.Tensor, target: torch.Tensor, patch: int = 14, stride: int = 14, rounding: bool = True,
         attention: bool = False):
    """As tests/s3_reference.py `step`: -> (features, (loss, l2, cos), {name: gradient}), float64."""
    p = REF.leaves(sd)
    feats = forward_features(p, img.double(), patch, stride, rounding, attention)
    loss, l2, cos = REF.loss_fn(feats, target.double())
    loss.backward()
    return feats.detach(), (loss.item(), l2.item(), cos.item()), {k: v.grad for k, v in p.items()}
