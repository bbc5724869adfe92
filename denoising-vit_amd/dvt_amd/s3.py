"""Host side of the stage-3 distillation step (csrc/dvt_stage3.hip, C ABI in include/dvt_stage3.h).

`Stage3Engine` owns four flat fp32 arenas on the device -- parameters, gradients and the two AdamW moments of a whole
DINOv2 ViT, in the layout `dvt_s3_param_offsets` reports, every tensor under its timm name and shape -- plus the
activation workspace.  `train_step` is forward + loss + backward of the student (main_distillation.py: the wrapper's
get_intermediate_layers(n=1, norm=True) features against the teacher's), gradients accumulated into `grads`; a batch
larger than the workspace budget runs in slices whose loss terms are normalised by the whole batch, so the accumulated
gradient is the whole batch's.  `adamw_step` is torch.optim.AdamW over the flat arenas (dvt_adamw_step).

A checkpoint whose position table has another grid than the run (`pos_grid`): `pos_embed` keeps the CHECKPOINT's shape in
all four arenas; every step resamples it to the run's grid (dvt_pos_resample_fwd, what timm's dynamic_img_size does in every
forward) and carries the gradient back through the transpose (dvt_pos_resample_bwd, what autograd does there).  The two
interpolation tables come from torch itself, once per engine (`pos_tables`).

`dtype="bfloat16"` (default "float32": exact fp32 throughout) is the opt-in mixed-precision step of include/dvt_stage3.h
(gemm_mode 1): the forward and data-gradient GEMMs of the blocks' four linear layers run on the extractor's bf16 MFMA GEMM with
operands rounded to bf16; weight gradients, arenas, activations and everything that is not one of those GEMMs stay fp32.
`attention="bfloat16"` on top of it (gemm_mode 3; refused with dtype="float32") runs the blocks' attention as the bf16 flash
attention of csrc/dvt_s3_attn.hip: no probabilities are kept, so the workspace per image shrinks and `slice_size` grows.
`weight_grad="bfloat16"` on top of dtype="bfloat16" (gemm_mode bit 4: modes 5 and 7; refused with dtype="float32") forms the
blocks' weight gradients dW = bf16(dy)^T bf16(x) on the bf16 split-K kernel of csrc/dvt_s3_wgrad.hip; bias gradients stay fp32.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from .arena import FlatAdamW
from .vit import VitConfig, vit_config

BLOCK_TENSORS = ["norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                 "ls1.gamma", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
                 "mlp.fc2.bias", "ls2.gamma"]

_P, _I = C.c_void_p, C.c_int
_lib.register_signatures({
    "dvt_s3_param_offsets": (_I, [C.POINTER(VitConfig), C.POINTER(C.c_int64)]),
    "dvt_s3_workspace_bytes": (C.c_int64, [C.POINTER(VitConfig), _I]),
    "dvt_s3_train_step": (_I, [C.POINTER(VitConfig), _P, _P, _P, _P, _P, _I, _P, C.c_int64, _P, _P]),
    "dvt_s3_train_slice": (_I, [C.POINTER(VitConfig), _P, _P, _P, _P, _P, _I, _I, _P, C.c_int64, _P, _P]),
    "dvt_pos_resample_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dvt_pos_resample_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dvt_s3_param_offsets_pos": (_I, [C.POINTER(VitConfig), _I, C.POINTER(C.c_int64)]),
    "dvt_s3_workspace_bytes_pos": (C.c_int64, [C.POINTER(VitConfig), _I, _I]),
    "dvt_s3_train_slice_pos": (_I, [C.POINTER(VitConfig), _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, C.c_int64, _P, _P]),
    "dvt_s3_workspace_bytes_mp": (C.c_int64, [C.POINTER(VitConfig), _I, _I, _I]),
    "dvt_s3_train_slice_pos_mp": (_I, [C.POINTER(VitConfig), _I, _P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _P, C.c_int64, _P,
                                       _P]),
    "dvt_s3_cast_bf16": (_I, [_P, _P, C.c_int64, _I, _P]),
    "dvt_s3_cast_bf16_t": (_I, [_P, _P, _I, _I, _P]),
    "dvt_s3_attn_operand_bytes": (C.c_int64, [_I, _I, _I]),
    "dvt_s3_attn_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "dvt_s3_attn_bwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
})

# gemm_mode of dvt_s3_train_slice_pos_mp is a bit set: Stage3Engine(dtype=) gives bit 0, Stage3Engine(attention=) bit 1,
# Stage3Engine(weight_grad=) bit 2
GEMM_MODES = {"float32": 0, "bfloat16": 1}
ATTENTION_MODES = {"float32": 0, "bfloat16": 2}
WEIGHT_GRAD_MODES = {"float32": 0, "bfloat16": 4}
ATTENTION_NEEDS_BF16 = ('attention="bfloat16" is built on the bf16 GEMM mode: it needs dtype="bfloat16" '
                        "(--attention bfloat16 needs --dtype bfloat16)")


def attn_fwd(qkv: torch.Tensor, batch: int, heads: int, n_valid: int):
    """dvt_s3_attn_fwd on its own: qkv fp32 [batch * Tp, 3 * 64 * heads] (device) -> (ao fp32 [batch * Tp, 64 * heads],
    lse fp32 [batch * heads, Tp] in log2 units, the bf16 operands [3, batch * heads, Tp, 64] that `attn_bwd` reads)."""
    _lib.require_cuda(qkv)
    R, C = qkv.shape[0], qkv.shape[1] // 3
    Tp = R // batch
    qkvb = torch.empty(3, batch * heads, Tp, 64, device=qkv.device, dtype=torch.bfloat16)
    ao = torch.empty(R, C, device=qkv.device, dtype=torch.float32)
    lse = torch.empty(batch * heads, Tp, device=qkv.device, dtype=torch.float32)
    _lib.check(_lib.lib().dvt_s3_attn_fwd(_lib.ptr(qkv), _lib.ptr(qkvb), _lib.ptr(ao), _lib.ptr(lse), batch, heads, n_valid, Tp,
                                          _lib.stream()), "dvt_s3_attn_fwd")
    return ao, lse, qkvb


def attn_bwd(qkvb: torch.Tensor, ao: torch.Tensor, dao: torch.Tensor, lse: torch.Tensor, batch: int, heads: int,
             n_valid: int) -> torch.Tensor:
    """dvt_s3_attn_bwd on its own: -> dqkv fp32 [batch * Tp, 3 * 64 * heads] (dq | dk | dv)."""
    _lib.require_cuda(qkvb, ao, dao, lse)
    R, C = ao.shape
    Tp = R // batch
    dqkv = torch.empty(R, 3 * C, device=ao.device, dtype=torch.float32)
    D = torch.empty(batch * heads, Tp, device=ao.device, dtype=torch.float32)
    _lib.check(_lib.lib().dvt_s3_attn_bwd(_lib.ptr(qkvb), _lib.ptr(ao), _lib.ptr(dao), _lib.ptr(lse), _lib.ptr(D), _lib.ptr(dqkv),
                                          batch, heads, n_valid, Tp, _lib.stream()), "dvt_s3_attn_bwd")
    return dqkv


WEIGHT_GRAD_NEEDS_BF16 = ('weight_grad="bfloat16" is built on the bf16 GEMM mode: it needs dtype="bfloat16" '
                          "(--weight_grad bfloat16 needs --dtype bfloat16)")


def wgrad_bf16(dy: torch.Tensor, x: torch.Tensor, dw: torch.Tensor | None = None, db: torch.Tensor | None = None,
               splits: int = 0):
    """dvt_s3_wgrad_bf16 on its own: dy fp32 [R, n], x fp32 [R, k] (device; R, n, k multiples of 128) -> (dw [n, k], db [n]) with
    dw = bf16(dy)^T bf16(x) in fp32 accumulation and db = colsum(dy) unrounded.  Given dw / db are ADDED to (accumulate = 1, both
    or neither); `splits`: 0 = the kernel's own split of the rows, >= 1 forces that many chunks."""
    _lib.require_cuda(dy, x, dw, db)
    if (dw is None) != (db is None):
        raise _lib.DvtError("wgrad_bf16 accumulates into both dw and db or into neither")
    R, n, k = dy.shape[0], dy.shape[1], x.shape[1]
    L = _lib.lib()
    nbytes = int(L.dvt_s3_wgrad_bf16_scratch_bytes(R, n, k, splits))
    if nbytes < 0 or x.shape[0] != R:
        raise _lib.DvtError(f"dvt_s3_wgrad_bf16: invalid shape R={R} n={n} k={k} splits={splits}")
    acc = dw is not None
    if not acc:
        dw = torch.empty(n, k, device=dy.device, dtype=torch.float32)
        db = torch.empty(n, device=dy.device, dtype=torch.float32)
    scratch = torch.empty(nbytes, device=dy.device, dtype=torch.uint8)
    _lib.check(L.dvt_s3_wgrad_bf16(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(scratch), nbytes, R, n, k,
                                   splits, int(acc), _lib.stream()), "dvt_s3_wgrad_bf16")
    return dw, db


def cast_bf16(x: torch.Tensor) -> torch.Tensor:
    """dvt_s3_cast_bf16 on its own: x fp32 [rows, n] (device, n % 4 == 0) -> bf16 [rows, n], round to nearest even."""
    _lib.require_cuda(x)
    y = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    _lib.check(_lib.lib().dvt_s3_cast_bf16(_lib.ptr(x), _lib.ptr(y), x.shape[0], x.shape[1], _lib.stream()), "dvt_s3_cast_bf16")
    return y


def cast_bf16_t(w: torch.Tensor) -> torch.Tensor:
    """dvt_s3_cast_bf16_t on its own: w fp32 [n, k] (device, n % 64 == k % 64 == 0) -> bf16 [k, n], the rounded transpose."""
    _lib.require_cuda(w)
    wt = torch.empty(w.shape[1], w.shape[0], device=w.device, dtype=torch.bfloat16)
    _lib.check(_lib.lib().dvt_s3_cast_bf16_t(_lib.ptr(w), _lib.ptr(wt), w.shape[0], w.shape[1], _lib.stream()),
               "dvt_s3_cast_bf16_t")
    return wt


def make_config(dim: int, depth: int, patch: int, stride: int, img_h: int, img_w: int, n_reg: int = 0) -> VitConfig:
    if dim not in (384, 768, 1024):
        raise NotImplementedError(f"the stage-3 step is built for dim 384 / 768 / 1024, got {dim}")
    return vit_config(dim, depth, patch, stride, img_h, img_w, n_reg, row_pad=128)


def pos_table(g0: int, g: int) -> torch.Tensor | None:
    """W [g, g0] (CPU fp32) with `F.interpolate(x, bicubic, antialias, align_corners=False)` along one axis of length g0
    resized to g == W @ x, read off torch itself by resizing the identity; None when g == g0 (a resize that keeps an axis'
    length is the identity along it).  Rows have at most 4 non-zero taps when enlarging, more when shrinking (10 at 37 ->
    16); everything outside that band is exactly zero."""
    import torch.nn.functional as F
    if g0 < 1 or g < 1:
        raise _lib.DvtError(f"a position grid needs at least one row, got {g0} -> {g}")
    if g == g0:
        return None
    return F.interpolate(torch.eye(g0, dtype=torch.float32)[None, None], size=(g, g0), mode="bicubic", antialias=True,
                         align_corners=False)[0, 0].contiguous()


def pos_tables(g0: int, gh: int, gw: int) -> tuple:
    """(Wy [gh, g0], Wx [gw, g0]) of the resample of a g0 x g0 table to gh x gw: per channel O = Wy P Wx^T."""
    return pos_table(g0, gh), pos_table(g0, gw)


def pos_resample(pos: torch.Tensor, wy, wx, grid: tuple, has_cls: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """dvt_pos_resample_fwd on its own: pos [has_cls + g0 g0, dim] (device fp32) -> [has_cls + gh gw, dim]; wy / wx are
    device tables (`pos_tables`) or None."""
    _lib.require_cuda(pos, wy, wx, out)
    gh, gw = grid
    dim, g0 = pos.shape[-1], math.isqrt(pos.shape[0] - has_cls)
    if out is None:
        out = torch.empty(has_cls + gh * gw, dim, device=pos.device, dtype=torch.float32)
    tmp = torch.empty(g0 * gw, dim, device=pos.device, dtype=torch.float32)
    _lib.check(_lib.lib().dvt_pos_resample_fwd(_lib.ptr(pos), _lib.ptr(out), _lib.ptr(wy), _lib.ptr(wx), _lib.ptr(tmp), g0,
                                               gh, gw, dim, has_cls, _lib.stream()), "dvt_pos_resample_fwd")
    return out


def pos_resample_bwd(dout: torch.Tensor, dpos: torch.Tensor, wy, wx, grid: tuple, has_cls: int) -> torch.Tensor:
    """dvt_pos_resample_bwd on its own: the transpose of `pos_resample` applied to dout [has_cls + gh gw, dim], ADDED to
    dpos [has_cls + g0 g0, dim]."""
    _lib.require_cuda(dout, dpos, wy, wx)
    gh, gw = grid
    dim, g0 = dpos.shape[-1], math.isqrt(dpos.shape[0] - has_cls)
    tmp = torch.empty(g0 * gw, dim, device=dpos.device, dtype=torch.float32)
    _lib.check(_lib.lib().dvt_pos_resample_bwd(_lib.ptr(dout), _lib.ptr(dpos), _lib.ptr(wy), _lib.ptr(wx), _lib.ptr(tmp), g0,
                                               gh, gw, dim, has_cls, _lib.stream()), "dvt_pos_resample_bwd")
    return dpos


def tensor_shapes(cfg: VitConfig, pos_grid: int | None = None) -> list:
    """Shapes of the timm tensors in arena order (names: `param_layout`).  `pos_grid`: the position table keeps a
    pos_grid x pos_grid patch part (the checkpoint's) instead of the run's grid."""
    d, f, p = cfg.dim, cfg.mlp_dim, cfg.patch
    block = [(d,), (d,), (3 * d, d), (3 * d,), (d, d), (d,), (d,), (d,), (d,), (f, d), (f,), (d, f), (d,), (d,)]
    n_pos = cfg.grid_h * cfg.grid_w if pos_grid is None else pos_grid * pos_grid
    return ([(d, 3, p, p), (d,), (1, 1, d), (1, cfg.n_prefix - 1, d), (1, cfg.pos_has_cls + n_pos, d)]
            + block * cfg.depth + [(d,), (d,)])


def param_names(cfg: VitConfig) -> list:
    return (["patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token", "reg_token", "pos_embed"]
            + [f"blocks.{b}.{t}" for b in range(cfg.depth) for t in BLOCK_TENSORS] + ["norm.weight", "norm.bias"])


def param_layout(cfg: VitConfig, pos_grid: int | None = None):
    """-> (total floats, {timm name: (offset, shape)}); `reg_token` only for models with register tokens."""
    n = 8 + 14 * cfg.depth
    out = (C.c_int64 * n)()
    if pos_grid is None:
        _lib.check(_lib.lib().dvt_s3_param_offsets(C.byref(cfg), out), "dvt_s3_param_offsets")
    else:
        _lib.check(_lib.lib().dvt_s3_param_offsets_pos(C.byref(cfg), int(pos_grid), out), "dvt_s3_param_offsets_pos")
    layout = {}
    for i, (name, shape) in enumerate(zip(param_names(cfg), tensor_shapes(cfg, pos_grid))):
        if name == "reg_token" and cfg.n_prefix == 1:
            continue
        layout[name] = (int(out[i]), shape)
    return int(out[n - 1]), layout


class Stage3Engine(FlatAdamW):
    def __init__(self, cfg: VitConfig, device: torch.device, pos_grid: int | None = None,
                 max_work_bytes: int | None = None, dtype: str = "float32", attention: str = "float32",
                 weight_grad: str = "float32"):
        """`pos_grid`: the grid g0 of the checkpoint's position table when `pos_embed` is to keep its [1, cls + g0 g0, dim]
        shape and be resampled to the run's grid in every step; None: the table is at the run's grid (the layout and the
        calls without a resample).
        `max_work_bytes`: budget of the activation workspace (default: 80 % of the device memory free after the
        arenas are allocated); `train_step` splits a batch into slices that fit.
        `dtype`: "float32" (exact fp32, the default) or "bfloat16": bf16 operands in the forward and data-gradient GEMMs of
        the blocks' linear layers (see the module's docstring); the arenas and the checkpoint are fp32 either way.
        `attention`: "float32" (the default: fp32 products, probabilities kept) or, with dtype="bfloat16" only, "bfloat16":
        the blocks' attention as bf16 flash attention, which keeps a log-sum-exp per row instead of the probabilities.
        `weight_grad`: "float32" (the default: exact fp32 weight gradients) or, with dtype="bfloat16" only, "bfloat16": the
        blocks' weight gradients from bf16-rounded dy and x on the split-K kernel; bias gradients stay fp32."""
        self.set_dtype(dtype, attention, weight_grad)
        if torch.device(device).type != "cuda":
            raise _lib.DvtError("the stage-3 engine needs a HIP device; there is no CPU fallback")
        self.cfg = cfg
        self.pos_grid = None if pos_grid is None else int(pos_grid)
        super().__init__(*param_layout(cfg, self.pos_grid), device)
        self._wy = self._wx = None
        if self.pos_grid is not None:
            self._wy, self._wx = (None if t is None else t.to(self.device)
                                  for t in pos_tables(self.pos_grid, cfg.grid_h, cfg.grid_w))
        self.loss = torch.zeros(4, device=self.device, dtype=torch.float32)
        self._slice_loss = torch.zeros(4, device=self.device, dtype=torch.float32)
        self.max_work_bytes = max_work_bytes

    def set_dtype(self, dtype: str, attention: str = "float32", weight_grad: str = "float32") -> None:
        """Arithmetic of the following steps.  The state is fp32 either way, so the dtype may change between steps (the
        interleaved A/B of tools/bench_stage3.py does); the workspace grows on demand."""
        if dtype not in GEMM_MODES:
            raise _lib.DvtError(f"the stage-3 step computes in {sorted(GEMM_MODES)}, got dtype={dtype!r}")
        if attention not in ATTENTION_MODES:
            raise _lib.DvtError(f"the stage-3 attention computes in {sorted(ATTENTION_MODES)}, got attention={attention!r}")
        if weight_grad not in WEIGHT_GRAD_MODES:
            raise _lib.DvtError(f"the stage-3 weight gradients compute in {sorted(WEIGHT_GRAD_MODES)}, got "
                                f"weight_grad={weight_grad!r}")
        if attention == "bfloat16" and dtype != "bfloat16":
            raise _lib.DvtError(ATTENTION_NEEDS_BF16)
        if weight_grad == "bfloat16" and dtype != "bfloat16":
            raise _lib.DvtError(WEIGHT_GRAD_NEEDS_BF16)
        self.dtype = dtype
        self.attention = attention
        self.weight_grad = weight_grad
        self.gemm_mode = GEMM_MODES[dtype] | ATTENTION_MODES[attention] | WEIGHT_GRAD_MODES[weight_grad]

    # ---- parameters -------------------------------------------------------------------------------
    def load_timm(self, state: dict) -> None:
        """Copy a timm VisionTransformer state dict (DINOv2 layout) into the parameter arena.  Its position table must be
        the engine's: the run's grid, or `pos_grid` when the engine was built with one."""
        v = self.views()
        missing = [k for k in v if k not in state]
        if missing:
            raise KeyError(f"ViT state dict lacks {missing}")
        for k, dst in v.items():
            src = state[k]
            if k == "pos_embed" and tuple(src.shape) != tuple(dst.shape):
                n_old = src.shape[-2] - self.cfg.pos_has_cls
                g0 = math.isqrt(max(n_old, 0))
                if src.dim() != 3 or g0 < 1 or g0 * g0 != n_old:
                    raise _lib.DvtError(f"pos_embed with {n_old} patch positions is not a square grid")
                raise NotImplementedError(
                    f"pos_embed {tuple(src.shape)} is not this engine's table {tuple(dst.shape)}: build the engine with "
                    f"pos_grid={g0} to train that table and resample it to the run's grid in every step")
            dst.copy_(src.detach().to(self.device, torch.float32).reshape(dst.shape))

    def state_dict(self) -> dict:
        """timm names -> CPU fp32 tensors (copies)."""
        return {k: t.detach().cpu().clone() for k, t in self.views().items()}

    # ---- kernels ----------------------------------------------------------------------------------
    def workspace_bytes(self, batch: int) -> int:
        if self.gemm_mode:
            n = int(_lib.lib().dvt_s3_workspace_bytes_mp(C.byref(self.cfg), batch, self._g0(), self.gemm_mode))
        elif self.pos_grid is None:
            n = int(_lib.lib().dvt_s3_workspace_bytes(C.byref(self.cfg), batch))
        else:
            n = int(_lib.lib().dvt_s3_workspace_bytes_pos(C.byref(self.cfg), batch, self.pos_grid))
        if n <= 0:
            raise _lib.DvtError("dvt_s3_workspace_bytes: invalid configuration")
        return n

    def _g0(self) -> int:
        """The table's grid for the `_mp` calls: `pos_grid`, or 0 for a table at the run's grid."""
        return 0 if self.pos_grid is None else self.pos_grid

    def slice_size(self, batch: int) -> int:
        """Images per slice for a batch of `batch`: the largest count whose workspace fits the budget."""
        budget = self.max_work_bytes
        if budget is None:
            free, _ = torch.cuda.mem_get_info(self.device)
            budget = int(0.8 * free) + (self._work.numel() if self._work is not None else 0)
        need = self.workspace_bytes(1)
        if need > budget:
            raise _lib.DvtError(f"one image needs {need} bytes of stage-3 workspace, {budget} are available")
        b = batch
        while b > 1 and self.workspace_bytes(b) > budget:
            b = max(1, min(b - 1, budget // need))
        return b

    def _check(self, img: torch.Tensor, target: torch.Tensor, feat: torch.Tensor | None):
        _lib.require_cuda(img, target, feat)
        c = self.cfg
        if img.dtype != torch.float32 or not img.is_contiguous() or tuple(img.shape[1:]) != (3, c.img_h, c.img_w):
            raise _lib.DvtError(f"expected a contiguous fp32 image batch [B, 3, {c.img_h}, {c.img_w}], got "
                                f"{tuple(img.shape)} {img.dtype}")
        want = (img.shape[0], c.grid_h, c.grid_w, c.dim)
        for name, t in (("target", target), ("feat", feat)):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != want):
                raise _lib.DvtError(f"{name} must be a contiguous fp32 {list(want)} tensor, got {tuple(t.shape)} {t.dtype}")

    def train_step(self, img: torch.Tensor, target: torch.Tensor, feat: torch.Tensor | None = None,
                   micro_batch: int | None = None) -> torch.Tensor:
        """Gradients of this batch are ADDED to `self.grads`; returns the device tensor [loss, l2_loss,
        cosine_similarity_loss, 0] of the whole batch (no synchronisation).  `feat` receives the student features.
        `micro_batch`: images per slice (default: as many as the workspace budget allows)."""
        self._check(img, target, feat)
        B = img.shape[0]
        mb = self.slice_size(B) if micro_batch is None else max(1, min(int(micro_batch), B))
        w = self._workspace(self.workspace_bytes(mb))
        L = _lib.lib()

        def run_slice(im, tg, ft, n, loss):
            if self.gemm_mode:
                return L.dvt_s3_train_slice_pos_mp(C.byref(self.cfg), self._g0(), _lib.ptr(self._wy), _lib.ptr(self._wx),
                                                   self.gemm_mode, _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(im),
                                                   _lib.ptr(tg), _lib.ptr(ft), n, B, _lib.ptr(w), w.numel(), _lib.ptr(loss),
                                                   _lib.stream())
            if self.pos_grid is None:
                return L.dvt_s3_train_slice(C.byref(self.cfg), _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(im),
                                            _lib.ptr(tg), _lib.ptr(ft), n, B, _lib.ptr(w), w.numel(), _lib.ptr(loss),
                                            _lib.stream())
            return L.dvt_s3_train_slice_pos(C.byref(self.cfg), self.pos_grid, _lib.ptr(self._wy), _lib.ptr(self._wx),
                                            _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(im), _lib.ptr(tg),
                                            _lib.ptr(ft), n, B, _lib.ptr(w), w.numel(), _lib.ptr(loss), _lib.stream())

        if mb >= B and self.pos_grid is None and not self.gemm_mode:
            _lib.check(L.dvt_s3_train_step(C.byref(self.cfg), _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(img),
                                           _lib.ptr(target), _lib.ptr(feat), B, _lib.ptr(w), w.numel(),
                                           _lib.ptr(self.loss), _lib.stream()), "dvt_s3_train_step")
            return self.loss
        if mb >= B:  # norm_batch == batch: the whole step
            _lib.check(run_slice(img, target, feat, B, self.loss), "dvt_s3_train_slice_pos(_mp)")
            return self.loss
        l2 = torch.zeros((), device=self.device)
        cos = torch.zeros((), device=self.device)
        for b0 in range(0, B, mb):
            n = min(mb, B - b0)
            _lib.check(run_slice(img[b0:], target[b0:], None if feat is None else feat[b0:], n, self._slice_loss),
                       "dvt_s3_train_slice")
            l2 += self._slice_loss[1]
            cos += 1.0 - self._slice_loss[2]
        self.loss.copy_(torch.stack([l2 + 1.0 - cos, l2, 1.0 - cos, torch.zeros_like(l2)]))
        return self.loss
