"""Comparator of the stage-2 training step's opt-in bf16 modes (tests helper, CPU; include/dvt_stage2.h
`dvt_s2_train_step_mp`): the `Denoiser` step of oracle/stage2.py in float64 in which each block's four
linear layers (qkv, proj, fc1, fc2) round what the mode rounds and nothing else --

    gemm_mode 1, 3    `MixedLinear` of tests/s3_bf16_reference.py: bf16 operands in the forward and the data gradient, weight
                      and bias gradients from the unrounded dy and x
    gemm_mode 5, 7    `WgradLinear` of tests/s3_wgrad_reference.py: the weight gradient from the rounded dy and x too
    gemm_mode 3, 7    `FlashAttention` and `qkv_bias` of tests/s3_attn_reference.py between them: the bf16 flash attention, and
                      the k third of each qkv bias a constant of the step

-- with every product exact (float64) and pos_embed, LayerNorm, GELU, the residual adds and the loss untouched.  `rounding=False`
switches every rounding off: plain float64 autograd, which tests/test_stage2_bf16_cpu.py holds to the oracle's own step."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import stage2 as O
from tests import s3_attn_reference as ATT
from tests import s3_bf16_reference as MP
from tests import s3_wgrad_reference as WG

MODES = (1, 3, 5, 7)


def leaves(sd: dict) -> dict:
    """The state dict (`pos_embed`, `denoiser.<tensor>` or `denoiser.<block>.<tensor>`) as float64 leaves."""
    return {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}


def n_blocks(sd: dict) -> int:
    idx = [k.split(".")[1] for k in sd if k.startswith("denoiser.")]
    return 1 + max(int(i) for i in idx) if idx[0].isdigit() else 1


def forward(p: dict, x: torch.Tensor, mode: int, rounding: bool = True, eps: float = 1e-6) -> torch.Tensor:
    """oracle/stage2.py `Denoiser.forward` on x [B, h, w, C] (float64) with the parameters `p` under gemm_mode `mode`."""
    if mode not in MODES:
        raise ValueError(f"the comparator restates gemm_modes {MODES}, got {mode}")
    B, h, w, C = x.shape
    heads, nb = C // 64, n_blocks(p)
    linear = WG.WgradLinear if mode & 4 else MP.MixedLinear
    attention = bool(mode & 2)
    y = x.reshape(B, h * w, C)
    if "pos_embed" in p:
        y = y + p["pos_embed"]
    for i in range(nb):
        pre = "denoiser." if nb == 1 and "denoiser.norm1.weight" in p else f"denoiser.{i}."
        lin = lambda t, name: linear.apply(t, p[pre + name + ".weight"], p[pre + name + ".bias"], rounding)  # noqa: E731
        n1 = F.layer_norm(y, (C,), p[pre + "norm1.weight"], p[pre + "norm1.bias"], eps)
        qb = p[pre + "attn.qkv.bias"]
        qkv = linear.apply(n1, p[pre + "attn.qkv.weight"], ATT.qkv_bias(qb, rounding) if attention else qb, rounding)
        q, k, v = qkv.reshape(B, -1, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)
        if attention:
            a = ATT.attention(q, k, v, rounding)
        else:
            a = torch.softmax((q * 64 ** -0.5) @ k.transpose(-2, -1), dim=-1) @ v
        y = y + lin(a.transpose(1, 2).reshape(B, -1, C), "attn.proj")
        n2 = F.layer_norm(y, (C,), p[pre + "norm2.weight"], p[pre + "norm2.bias"], eps)
        y = y + lin(F.gelu(lin(n2, "mlp.fc1")), "mlp.fc2")
    return y.reshape(B, h, w, C)


def step(sd: dict, x: torch.Tensor, target: torch.Tensor, mode: int, rounding: bool = True):
    """One step -> (pred, (loss, l2, cos), {name: gradient}), float64."""
    p = leaves(sd)
    pred = forward(p, x.double(), mode, rounding)
    loss, l2, cos = O.loss_fn(pred, target.double())
    loss.backward()
    return pred.detach(), (loss.item(), l2.item(), cos.item()), {k: v.grad for k, v in p.items()}


def oracle_step(ref: O.Denoiser, x: torch.Tensor, target: torch.Tensor):
    """The oracle's own autograd step in float64 on a copy of `ref` -> the same triple."""
    import copy
    m = copy.deepcopy(ref).double()
    m.zero_grad()
    pred = m(x.double())
    loss, l2, cos = O.loss_fn(pred, target.double())
    loss.backward()
    return pred.detach(), (loss.item(), l2.item(), cos.item()), {k: v.grad for k, v in m.named_parameters()}
