"""Autograd reference of the stage-3 step (tests helper, CPU): the student's features are oracle/vit.py's
`forward_features` -- plain torch, so calling it on leaf tensors that require grad gives autograd's gradients --, the
loss is main_distillation.py's `F.mse_loss(pred, target) + 1 - F.cosine_similarity(pred, target, dim=-1).mean()`."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import vit as OV


def loss_fn(pred: torch.Tensor, target: torch.Tensor):
    l2 = F.mse_loss(pred, target)
    cos = 1 - F.cosine_similarity(pred, target, dim=-1).mean()
    return l2 + cos, l2, cos


def leaves(sd: dict, dtype=torch.float64) -> dict:
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}


def step(sd: dict, img: torch.Tensor, target: torch.Tensor, patch: int = 14, stride: int = 14, dtype=torch.float64):
    """-> (features, (loss, l2, cos), {name: gradient}) of one forward + backward in `dtype`."""
    p = leaves(sd, dtype)
    feats = OV.forward_features(p, img.to(dtype), patch=patch, stride=stride)
    loss, l2, cos = loss_fn(feats, target.to(dtype))
    loss.backward()
    return feats.detach(), (loss.item(), l2.item(), cos.item()), {k: v.grad for k, v in p.items()}
