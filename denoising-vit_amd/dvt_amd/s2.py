"""Host side of the stage-2 denoiser kernels (csrc/dvt_stage2.hip, C ABI in include/dvt_stage2.h).

`Stage2Engine` owns four flat fp32 arenas on the device -- parameters, gradients and the two AdamW moments,
all in the layout `dvt_s2_param_offsets` reports -- plus the activation workspace, and exposes the three
operations the reference's stage-2 loop consists of (main_denoiser.py:212-221): `forward`, `train_step`
(forward + loss + backward, gradients accumulated into the flat gradient arena) and `adamw_step`.  A
data-parallel trainer all-reduces `engine.grads` between the last two (one flat RCCL all-reduce per step).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from .arena import FlatAdamW

BLOCK_TENSORS = ["norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight",
                 "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias",
                 "mlp.fc2.weight", "mlp.fc2.bias"]
MAX_BLOCKS = 8


class S2Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dim", "heads", "mlp_dim", "tokens", "tokens_pad", "n_blocks",
                                         "enable_pe")] + [("ln_eps", C.c_float)]


_P, _I = C.c_void_p, C.c_int
_lib.register_signatures({
    "dvt_s2_param_offsets": (_I, [C.POINTER(S2Config), C.POINTER(C.c_int64)]),
    "dvt_s2_workspace_bytes": (C.c_int64, [C.POINTER(S2Config), _I, _I]),
    "dvt_s2_forward": (_I, [C.POINTER(S2Config), _P, _P, _P, _I, _P, C.c_int64, _P]),
    "dvt_s2_train_step": (_I, [C.POINTER(S2Config), _P, _P, _P, _P, _P, _I, _P, C.c_int64, _P, _P]),
    "dvt_s2_workspace_bytes_mp": (C.c_int64, [C.POINTER(S2Config), _I, _I, _I]),
    "dvt_s2_train_step_mp": (_I, [C.POINTER(S2Config), _P, _P, _P, _P, _P, _I, _P, C.c_int64, _P, _P, _I]),
})

# gemm_mode of dvt_s2_train_step_mp is the stage-3 step's bit set: Stage2Engine(dtype=) gives bit 0, Stage2Engine(attention=)
# bit 1, Stage2Engine(weight_grad=) bit 2
GEMM_MODES = {"float32": 0, "bfloat16": 1}
ATTENTION_MODES = {"float32": 0, "bfloat16": 2}
WEIGHT_GRAD_MODES = {"float32": 0, "bfloat16": 4}
ATTENTION_NEEDS_BF16 = ('attention="bfloat16" is built on the bf16 GEMM mode: it needs dtype="bfloat16" '
                        "(--attention bfloat16 needs --dtype bfloat16)")
WEIGHT_GRAD_NEEDS_BF16 = ('weight_grad="bfloat16" is built on the bf16 GEMM mode: it needs dtype="bfloat16" '
                          "(--weight_grad bfloat16 needs --dtype bfloat16)")
BF16_ROW_PAD = 128  # the bf16 kernels walk 128-row tiles of an image's rows


def gemm_mode(dtype: str = "float32", attention: str = "float32", weight_grad: str = "float32") -> int:
    """The three switches as one gemm_mode; a value outside the choices, or attention / weight_grad without the bf16 GEMM mode
    under them, is refused by name (no device is touched)."""
    if dtype not in GEMM_MODES:
        raise _lib.DvtError(f"the stage-2 step computes in {sorted(GEMM_MODES)}, got dtype={dtype!r}")
    if attention not in ATTENTION_MODES:
        raise _lib.DvtError(f"the stage-2 attention computes in {sorted(ATTENTION_MODES)}, got attention={attention!r}")
    if weight_grad not in WEIGHT_GRAD_MODES:
        raise _lib.DvtError(f"the stage-2 weight gradients compute in {sorted(WEIGHT_GRAD_MODES)}, got "
                            f"weight_grad={weight_grad!r}")
    if attention == "bfloat16" and dtype != "bfloat16":
        raise _lib.DvtError(ATTENTION_NEEDS_BF16)
    if weight_grad == "bfloat16" and dtype != "bfloat16":
        raise _lib.DvtError(WEIGHT_GRAD_NEEDS_BF16)
    return GEMM_MODES[dtype] | ATTENTION_MODES[attention] | WEIGHT_GRAD_MODES[weight_grad]


def make_config(feat_dim: int, tokens: int, num_blocks: int = 1, enable_pe: bool = True, row_pad: int = 64) -> S2Config:
    """`row_pad`: an image's rows are padded to a multiple of it -- 64 (the default: what the fp32 step has always used) or
    128, which the bf16 modes of the training step need."""
    if feat_dim not in (384, 768, 1024):
        raise NotImplementedError(f"stage-2 kernels are built for feat_dim 384 / 768 / 1024, got {feat_dim}")
    if not 1 <= num_blocks <= MAX_BLOCKS:
        raise ValueError(f"num_blocks must be in [1, {MAX_BLOCKS}]")
    c = S2Config()
    c.dim, c.heads, c.mlp_dim = feat_dim, feat_dim // 64, 4 * feat_dim
    if row_pad not in (64, 128):
        raise ValueError(f"row_pad must be 64 or 128, got {row_pad}")
    c.tokens, c.tokens_pad = tokens, (tokens + row_pad - 1) // row_pad * row_pad
    c.n_blocks, c.enable_pe, c.ln_eps = num_blocks, int(bool(enable_pe)), 1e-6
    return c


def tensor_shapes(cfg: S2Config) -> list:
    d, f = cfg.dim, cfg.mlp_dim
    return [(d,), (d,), (3 * d, d), (3 * d,), (d, d), (d,), (d,), (d,), (f, d), (f,), (d, f), (d,)]


def param_layout(cfg: S2Config):
    """-> (total floats, {name: (offset, shape)}) with the reference's state-dict names
    (`pos_embed`, `denoiser.<tensor>` or `denoiser.<block>.<tensor>` for num_blocks > 1)."""
    out = (C.c_int64 * (2 + 12 * cfg.n_blocks))()
    _lib.check(_lib.lib().dvt_s2_param_offsets(C.byref(cfg), out), "dvt_s2_param_offsets")
    names = {}
    if cfg.enable_pe:
        names["pos_embed"] = (out[0], (1, cfg.tokens, cfg.dim))
    shapes = tensor_shapes(cfg)
    for b in range(cfg.n_blocks):
        prefix = "denoiser." if cfg.n_blocks == 1 else f"denoiser.{b}."
        for i, t in enumerate(BLOCK_TENSORS):
            names[prefix + t] = (out[1 + 12 * b + i], shapes[i])
    return int(out[1 + 12 * cfg.n_blocks]), names


class Stage2Engine(FlatAdamW):
    def __init__(self, cfg: S2Config, device: torch.device, inference_only: bool = False, dtype: str = "float32",
                 attention: str = "float32", weight_grad: str = "float32"):
        """inference_only: a parameter arena and nothing else (no gradient / moment arenas: 3/4 of the memory) --
        what `Denoiser._engine_for` needs for its resized copies.
        `dtype`, `attention`, `weight_grad`: arithmetic of `train_step`, as `Stage3Engine`'s -- "float32" each (the default:
        exact fp32) or, opt-in, "bfloat16": bf16 operands in the forward and data-gradient GEMMs of the blocks' linear layers
        (`dtype`), on top of it the bf16 flash attention, which keeps no [tokens, tokens] matrix (`attention`), and the bf16
        split-K weight gradients (`weight_grad`).  `forward`, the arenas and the checkpoint are fp32 either way.  A bf16 engine
        needs a config built with row_pad=128."""
        self.set_dtype(dtype, attention, weight_grad)
        if torch.device(device).type != "cuda":
            raise _lib.DvtError("the stage-2 engine needs a HIP device; there is no CPU fallback")
        self.cfg = cfg
        super().__init__(*param_layout(cfg), device, inference_only)
        self.loss = torch.zeros(4, device=self.device, dtype=torch.float32)
        self.param_version = 0  # bumped by everything that writes the parameter arena through this engine
        self._work = {}  # (batch, training) -> buffer: one per mode, sized exactly (not the base's single grow-only one)

    def set_dtype(self, dtype: str, attention: str = "float32", weight_grad: str = "float32") -> None:
        """Arithmetic of the following training steps.  The state is fp32 either way, so it may change between steps (the
        interleaved A/B of tools/bench_stage2.py does)."""
        mode = gemm_mode(dtype, attention, weight_grad)
        self.dtype, self.attention, self.weight_grad, self.gemm_mode = dtype, attention, weight_grad, mode
        self._work = {k: v for k, v in getattr(self, "_work", {}).items() if not k[1]}  # the training buffer is the mode's

    # ---- parameters -------------------------------------------------------------------------------
    def init_parameters(self, generator: torch.Generator | None = None) -> None:
        """The reference's initial state: standalone timm `Block`s keep the `nn.Linear` / `nn.LayerNorm`
        defaults (kaiming-uniform(a=sqrt 5) weights and U(+-1/sqrt(fan_in)) biases; ones / zeros), and
        pos_embed = randn * 0.02 (online_denoiser.py:24-57).  Drawn on the host, then uploaded."""
        g = generator
        for name, v in self.views().items():
            if name == "pos_embed":
                t = torch.randn(v.shape, generator=g) * 0.02
            elif name.endswith("norm1.weight") or name.endswith("norm2.weight"):
                t = torch.ones(v.shape)
            elif name.endswith("norm1.bias") or name.endswith("norm2.bias"):
                t = torch.zeros(v.shape)
            else:
                wname = name[:-len("bias")] + "weight" if name.endswith("bias") else name
                fan_in = self.layout[wname][1][1]
                bound = 1.0 / math.sqrt(fan_in)
                t = (torch.rand(v.shape, generator=g) * 2 - 1) * bound
            v.copy_(t.to(self.device))

    def load_named(self, state: dict) -> None:
        v = self.views()
        missing = [k for k in v if k not in state]
        if missing:
            raise KeyError(f"stage-2 checkpoint lacks {missing}")
        for k, dst in v.items():
            dst.copy_(state[k].to(self.device, torch.float32).reshape(dst.shape))
        self.param_version += 1

    # ---- kernels ----------------------------------------------------------------------------------
    def _workspace(self, batch: int, training: bool) -> torch.Tensor:
        key = (batch, training)
        if key not in self._work:
            n = self.workspace_bytes(batch, training)
            self._work = {k: v for k, v in self._work.items() if k[1] != training}  # one per mode
            self._work[key] = torch.empty(n, device=self.device, dtype=torch.uint8)
        return self._work[key]

    def workspace_bytes(self, batch: int, training: bool = True) -> int:
        if training and self.gemm_mode:
            n = int(_lib.lib().dvt_s2_workspace_bytes_mp(C.byref(self.cfg), batch, 1, self.gemm_mode))
            if n <= 0:
                raise _lib.DvtError(f"dvt_s2_workspace_bytes_mp: gemm_mode {self.gemm_mode} needs tokens_pad % 128 == 0 "
                                    f"(make_config(..., row_pad={BF16_ROW_PAD})) and mlp_dim % 128 == 0, got tokens_pad "
                                    f"{self.cfg.tokens_pad}, mlp_dim {self.cfg.mlp_dim}")
            return n
        n = int(_lib.lib().dvt_s2_workspace_bytes(C.byref(self.cfg), batch, int(training)))
        if n <= 0:
            raise _lib.DvtError("dvt_s2_workspace_bytes: invalid configuration")
        return n

    def _check_io(self, *ts):
        _lib.require_cuda(*ts)
        for t in ts:
            if t is None:
                continue
            if t.dtype != torch.float32 or not t.is_contiguous() or t.shape[1:] != (self.cfg.tokens, self.cfg.dim):
                raise _lib.DvtError(f"expected contiguous fp32 [batch, {self.cfg.tokens}, {self.cfg.dim}], got "
                                    f"{tuple(t.shape)} {t.dtype}")

    def forward(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        self._check_io(x, out)
        out = torch.empty_like(x) if out is None else out
        w = self._workspace(x.shape[0], False)
        _lib.check(_lib.lib().dvt_s2_forward(C.byref(self.cfg), _lib.ptr(self.params), _lib.ptr(x), _lib.ptr(out),
                                             x.shape[0], _lib.ptr(w), w.numel(), _lib.stream()), "dvt_s2_forward")
        return out

    def train_step(self, x: torch.Tensor, target: torch.Tensor, pred: torch.Tensor | None = None) -> torch.Tensor:
        """Gradients of this batch are ADDED to `self.grads`; returns the device tensor
        [loss, l2_loss, cosine_similarity_loss, 0] (no synchronisation)."""
        self._check_io(x, target, pred)
        if self.inference_only:
            raise _lib.DvtError("this engine was built inference_only (no gradient arena)")
        if target.shape != x.shape:
            raise _lib.DvtError("target and input shapes differ")
        w = self._workspace(x.shape[0], True)
        if self.gemm_mode:
            _lib.check(_lib.lib().dvt_s2_train_step_mp(C.byref(self.cfg), _lib.ptr(self.params), _lib.ptr(self.grads),
                                                       _lib.ptr(x), _lib.ptr(target), _lib.ptr(pred), x.shape[0], _lib.ptr(w),
                                                       w.numel(), _lib.ptr(self.loss), _lib.stream(), self.gemm_mode),
                       "dvt_s2_train_step_mp")
            return self.loss
        _lib.check(_lib.lib().dvt_s2_train_step(C.byref(self.cfg), _lib.ptr(self.params), _lib.ptr(self.grads),
                                                _lib.ptr(x), _lib.ptr(target), _lib.ptr(pred), x.shape[0], _lib.ptr(w),
                                                w.numel(), _lib.ptr(self.loss), _lib.stream()), "dvt_s2_train_step")
        return self.loss

    def adamw_step(self, *args, **kwargs) -> None:
        super().adamw_step(*args, **kwargs)
        self.param_version += 1
