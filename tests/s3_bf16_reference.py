"""Comparator of the stage-3 step's opt-in bf16 mode (tests helper, CPU): the float64 step of tests/s3_reference.py in which
each of a block's four linear layers (qkv, proj, fc1, fc2) is a `torch.autograd.Function` that does what the mode does and
nothing else --

    forward         y  = bf16(x)  . bf16(W)^T + b
    data gradient   dx = bf16(dy) . bf16(W)
    weight gradient dW = dy^T . x,  db = colsum(dy)        from the UNROUNDED dy and x

-- with the products, and everything around them (patch embedding, position table, LayerNorm, attention, softmax, GELU,
LayerScale, the loss), in float64.  bf16(.) rounds through fp32 to bf16, round to nearest even (the step's operands are
fp32 values), and goes back to float64.  It is a correct evaluation of the mode's arithmetic with exact accumulation: its
distance from plain float64 autograd is the error the ROUNDING makes, the yardstick the GPU tests hold the kernels to.

`rounding=False` switches the rounding off: the same code is then plain float64 autograd, and tests/test_stage3_bf16_cpu.py
holds it to tests/s3_reference.py -- the forward is restated here (oracle/vit.py calls F.linear directly), so that check is
what ties the restatement to the oracle."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import vit as OV
from tests import s3_reference as REF


def bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


class MixedLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, rounding):
        ctx.save_for_backward(x, w)
        ctx.rounding = rounding
        r = bf16 if rounding else (lambda t: t)
        return r(x) @ r(w).t() + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        r = bf16 if ctx.rounding else (lambda t: t)
        dx = r(dy) @ r(w)
        dy2, x2 = dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1])
        return dx, dy2.t() @ x2, dy2.sum(0), None


def forward_features(sd: dict, img: torch.Tensor, patch: int, stride: int, rounding: bool = True, eps: float = 1e-6):
    """oracle/vit.py `forward_features` (all blocks, final norm) with the four linear layers of a block as MixedLinear."""
    dim = sd["pos_embed"].shape[-1]
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    heads = dim // 64
    lin = lambda h, name: MixedLinear.apply(h, sd[name + ".weight"], sd[name + ".bias"], rounding)  # noqa: E731
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
        q, k, v = lin(h, p + "attn.qkv").reshape(B, -1, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)
        a = torch.softmax((q * 64 ** -0.5) @ k.transpose(-2, -1), dim=-1) @ v
        a = lin(a.transpose(1, 2).reshape(B, -1, dim), p + "attn.proj")
        x = x + sd[p + "ls1.gamma"] * a
        h = F.layer_norm(x, (dim,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
        h = lin(F.gelu(lin(h, p + "mlp.fc1")), p + "mlp.fc2")
        x = x + sd[p + "ls2.gamma"] * h
    x = F.layer_norm(x, (dim,), sd["norm.weight"], sd["norm.bias"], eps)
    return x[:, 1 + n_reg:].reshape(B, gh, gw, dim)


def step(sd: dict, img: torch.Tensor, target: torch.Tensor, patch: int = 14, stride: int = 14, rounding: bool = True):
    """As tests/s3_reference.py `step`: -> (features, (loss, l2, cos), {name: gradient}), float64."""
    p = REF.leaves(sd)
    feats = forward_features(p, img.double(), patch, stride, rounding)
    loss, l2, cos = REF.loss_fn(feats, target.double())
    loss.backward()
    return feats.detach(), (loss.item(), l2.item(), cos.item()), {k: v.grad for k, v in p.items()}
