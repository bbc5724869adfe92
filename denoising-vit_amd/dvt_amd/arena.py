"""The flat AdamW arena the four trainers share, and the torch checkpoint layout of its moments.

`FlatAdamW` is the base of `Stage2Engine`, `Stage3Engine`, `SegHeadEngine` and `DepthHeadEngine`: four flat fp32 arenas on
the device -- parameters, gradients and the two AdamW moments, all in one `layout` of `{name: (offset, shape)}` -- the step
counter, and `dvt_adamw_step` (csrc/dvt_adam.hip) over them.  The free functions build and read
`torch.optim.AdamW.state_dict()` from the flat moments; they touch only `views`, `exp_avg`, `exp_avg_sq` and `step`, so
anything with those four works (the CPU stand-ins of the tests).
"""
from __future__ import annotations

import ctypes as C
import math
import os

import torch

from . import _lib

_P, _I, _F = C.c_void_p, C.c_int, C.c_float
_lib.register_signatures({
    "dvt_adamw_step": (_I, [_P, _P, _P, _P, C.c_int64, _F, _F, _F, _F, _F, _I, _F, _P]),
})

# the keys torch >= 2 adds to an AdamW param group, at their defaults (what the stage-2 and stage-3 checkpoints carry)
TORCH2_GROUP_DEFAULTS = {"maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None}


class FlatAdamW:
    WEIGHT_DECAY = None  # an engine whose reference config fixes the decay names it here; the others pass it per step

    def __init__(self, total: int, layout: dict, device, inference_only: bool = False):
        """inference_only: a parameter arena and nothing else (no gradient / moment arenas: 3/4 of the memory)."""
        self.total, self.layout, self.device = int(total), layout, torch.device(device)
        z = lambda: torch.zeros(self.total, device=self.device, dtype=torch.float32)  # noqa: E731
        self.params = z()
        self.inference_only = inference_only
        self.grads = self.exp_avg = self.exp_avg_sq = None
        if not inference_only:
            self.grads, self.exp_avg, self.exp_avg_sq = z(), z(), z()
        self.step = 0
        self._work = None

    def views(self, arena: torch.Tensor | None = None) -> dict:
        arena = self.params if arena is None else arena
        return {n: arena[o:o + math.prod(s)].view(s) for n, (o, s) in self.layout.items()}

    def _workspace(self, nbytes: int) -> torch.Tensor:
        """Grow-only: the old buffer is dropped before the larger one is allocated."""
        if self._work is None or self._work.numel() < nbytes:
            self._work = None
            self._work = torch.empty(nbytes, device=self.device, dtype=torch.uint8)
        return self._work

    def adamw_step(self, lr: float, weight_decay: float | None = None, betas=(0.9, 0.999), eps: float = 1e-8,
                   grad_scale: float = 1.0) -> None:
        """torch.optim.AdamW over every tensor of the arena (one param group); zeroes `grads`."""
        if self.inference_only:
            raise _lib.DvtError("this engine was built inference_only (no optimizer state)")
        weight_decay = self.WEIGHT_DECAY if weight_decay is None else weight_decay
        self.step += 1
        _lib.check(_lib.lib().dvt_adamw_step(_lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.exp_avg),
                                             _lib.ptr(self.exp_avg_sq), self.total, lr, betas[0], betas[1], eps,
                                             weight_decay, self.step, grad_scale, _lib.stream()), "dvt_adamw_step")

    def optimizer_state(self) -> dict:
        return {"step": self.step, "exp_avg": self.exp_avg.cpu().clone(), "exp_avg_sq": self.exp_avg_sq.cpu().clone()}

    def load_optimizer_state(self, st: dict) -> None:
        self.step = int(st["step"])
        self.exp_avg.copy_(st["exp_avg"])
        self.exp_avg_sq.copy_(st["exp_avg_sq"])


# ---- torch.optim.AdamW.state_dict() over the flat moments ----------------------------------------------------------
def adamw_group(lr: float, weight_decay: float, betas=(0.9, 0.999), **extra) -> dict:
    """One AdamW param group without its `params`: the keys every torch has, then the writer's own (`extra`)."""
    return {"lr": lr, "betas": tuple(betas), "eps": 1e-8, "weight_decay": weight_decay, "amsgrad": False, **extra}


def adamw_state_dict(eng, names, group: dict, empty_before_first_step: bool = False) -> dict:
    """`{"state", "param_groups"}` over the tensors `names` in that order; `group` (see `adamw_group`) gets its `params`.
    empty_before_first_step: no state while `eng.step == 0`, as torch's own optimizer has none before its first step."""
    m, v = eng.views(eng.exp_avg), eng.views(eng.exp_avg_sq)
    state = {}
    if eng.step or not empty_before_first_step:
        state = {i: {"step": torch.tensor(float(eng.step)), "exp_avg": m[n].detach().cpu().clone(),
                     "exp_avg_sq": v[n].detach().cpu().clone()} for i, n in enumerate(names)}
    return {"state": state, "param_groups": [{**group, "params": list(range(len(names)))}]}


def load_adamw_state(eng, names, state: dict) -> None:
    """The reverse: `state` is the optimizer's `state_dict()`; its per-tensor keys may be int or str, and a tensor without
    an entry (a checkpoint saved before the first step) keeps its moments."""
    m, v = eng.views(eng.exp_avg), eng.views(eng.exp_avg_sq)
    for i, n in enumerate(names):
        s = state["state"].get(i, state["state"].get(str(i)))
        if s is None:
            continue
        m[n].copy_(s["exp_avg"].reshape(m[n].shape))
        v[n].copy_(s["exp_avg_sq"].reshape(v[n].shape))
        eng.step = int(float(s["step"]))


def link_latest(path: str, latest: str) -> None:
    """`latest` becomes a symlink to `path` (absolute), replacing the one of the previous checkpoint."""
    try:
        os.remove(latest)
    except FileNotFoundError:
        pass
    os.symlink(os.path.abspath(path), latest)
