"""Comparator of the stage-3 step's bf16 flash attention (tests helper, CPU; include/dvt_stage3.h gemm_mode 3,
csrc/dvt_s3_attn.hip): float64 attention, forward and backward, that rounds exactly what the mode rounds and nothing else --

    forward    q' = bf16(q log2(e) / 8),  kb = bf16(k),  vb = bf16(v)
               s = q' kb^T (log2 units),  lse = log2 sum_k 2^s,  P = 2^(s - lse)
               ao = (sum over the 32-key tiles t of  2^(m_t - m) bf16(2^(s - m_t)) vb) / sum_k 2^(s - m)
               -- what reaches the P v product is P relative to the RUNNING row maximum m_t of the flash loop (the maximum
               over the tiles up to t; m the final one), rounded there, rescaled and normalised unrounded: the kernel cannot
               round the normalised P, it does not know the sum yet.  With one tile: ao = bf16(2^(s - m)) vb / sum 2^(s - m)
    backward   D = rowsum(dao (.) ao)            from the UNROUNDED dao and ao
               dv = bf16(P)^T bf16(dao),  dP = bf16(dao) vb^T,  dS = P (.) (dP - D)
               dq = bf16(dS) kb / 8,  dk = ln 2 bf16(dS)^T q'   (= bf16(dS)^T q / 8 without the rounding of q')

-- with every product, lse and D exact (float64).  bf16(.) is tests/s3_bf16_reference.py's: through fp32, round to nearest
even.  `rounding=False` makes it plain softmax(q k^T / 8) v with a hand-written backward, which tests/test_stage3_attn_cpu.py
holds to autograd and, as a whole step, to tests/s3_reference.py.

`tiled_backward` restates the SHAPE of the two backward kernels in float64 without any rounding: one pass per block of 128
keys sweeping 32-query tiles (dk, dv), one pass per block of 128 queries sweeping 32-key tiles (dq), P recomputed from lse in
both, keys and queries >= T masked -- the recompute identity and the split, tested against autograd.

`forward_features` / `step` are tests/s3_bf16_reference.py's with this attention between its MixedLinear layers, and with
the k third of each qkv bias held constant, as the mode holds it (`qkv_bias`)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import vit as OV
from tests import s3_bf16_reference as MP
from tests import s3_reference as REF

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
Q_PRESCALE = 0.125 * LOG2E


def _ident(t):
    return t


TILE = 32  # keys per tile of the forward's flash loop (SA_T of csrc/dvt_s3_attn.hip)


def flash_forward(qs, kb, vb, r):
    """(ao, lse): the online-softmax loop over TILE-key tiles in float64, P rounded by `r` where it meets v."""
    s = qs @ kb.transpose(-1, -2)
    m = torch.full(s.shape[:-1] + (1,), -float("inf"), dtype=s.dtype)
    l = torch.zeros_like(m)
    acc = torch.zeros(s.shape[:-1] + (vb.shape[-1],), dtype=s.dtype)
    for t0 in range(0, s.shape[-1], TILE):
        st = s[..., t0:t0 + TILE]
        m_new = torch.maximum(m, st.amax(-1, keepdim=True))
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(st - m_new)
        l = l * alpha + p.sum(-1, keepdim=True)
        acc = acc * alpha + r(p) @ vb[..., t0:t0 + TILE, :]
        m = m_new
    return acc / l, (m + torch.log2(l)).squeeze(-1)


def log2_sum_exp2(s: torch.Tensor) -> torch.Tensor:
    m = s.amax(-1, keepdim=True)
    return (m + torch.log2(torch.exp2(s - m).sum(-1, keepdim=True))).squeeze(-1)


class FlashAttention(torch.autograd.Function):
    """q, k, v [..., T, 64] float64 -> ao [..., T, 64]; see the module docstring."""

    @staticmethod
    def forward(ctx, q, k, v, rounding):
        r = MP.bf16 if rounding else _ident
        qs, kb, vb = r(q * Q_PRESCALE), r(k), r(v)
        ao, lse = flash_forward(qs, kb, vb, r)
        ctx.save_for_backward(qs, kb, vb, lse, ao)
        ctx.rounding = rounding
        return ao

    @staticmethod
    def backward(ctx, dao):
        qs, kb, vb, lse, ao = ctx.saved_tensors
        r = MP.bf16 if ctx.rounding else _ident
        p = torch.exp2(qs @ kb.transpose(-1, -2) - lse[..., None])  # recomputed, as the kernels do
        D = (dao * ao).sum(-1, keepdim=True)
        dob = r(dao)
        dv = r(p).transpose(-1, -2) @ dob
        ds = r(p * (dob @ vb.transpose(-1, -2) - D))
        dq = (ds @ kb) * 0.125
        dk = (ds.transpose(-1, -2) @ qs) * LN2
        return dq, dk, dv, None


def attention(q, k, v, rounding=True):
    return FlashAttention.apply(q, k, v, rounding)


def forward_lse(q, k, v, rounding=True):
    """(ao, lse in log2 units) without autograd."""
    r = MP.bf16 if rounding else _ident
    qs, kb, vb = r(q * Q_PRESCALE), r(k), r(v)
    return flash_forward(qs, kb, vb, r)


def tiled_backward(q, k, v, dao, n_valid, block=128, tile=32):
    """q, k, v, dao [H, Tp, 64] float64 (rows >= n_valid: padding) -> (ao, lse, dq, dk, dv), each [H, Tp, ..]: the forward
    over the valid keys, then the two backward passes of csrc/dvt_s3_attn.hip tile by tile, no rounding."""
    H, Tp, _ = q.shape
    T = n_valid
    qs = q * Q_PRESCALE
    s = qs[:, :T] @ k[:, :T].transpose(-1, -2)
    lse = torch.zeros(H, Tp, dtype=q.dtype)
    lse[:, :T] = log2_sum_exp2(s)
    ao = torch.zeros_like(q)
    ao[:, :T] = torch.exp2(s - lse[:, :T, None]) @ v[:, :T]
    D = (dao * ao).sum(-1)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
    nt = math.ceil(T / tile)

    def on(rows):  # mask of valid indices
        return (rows < T).to(q.dtype)

    for k0 in range(0, Tp, block):        # pass 1: a block of keys owns its dk, dv and sweeps the queries
        if k0 >= T:
            continue
        kk = torch.arange(k0, k0 + block)
        for t in range(nt):
            qq = torch.arange(t * tile, (t + 1) * tile)
            mask = on(qq)[:, None] * on(kk)[None, :]
            p = torch.exp2(qs[:, qq] @ k[:, kk].transpose(-1, -2) - lse[:, qq, None]) * mask
            ds = p * (dao[:, qq] @ v[:, kk].transpose(-1, -2) - D[:, qq, None])
            dv[:, kk] += p.transpose(-1, -2) @ dao[:, qq]
            dk[:, kk] += (ds.transpose(-1, -2) @ qs[:, qq]) * LN2
    for q0 in range(0, Tp, block):        # pass 2: a block of queries owns its dq and sweeps the keys
        if q0 >= T:
            continue
        qq = torch.arange(q0, q0 + block)
        for t in range(nt):
            kk = torch.arange(t * tile, (t + 1) * tile)
            mask = on(qq)[:, None] * on(kk)[None, :]
            p = torch.exp2(qs[:, qq] @ k[:, kk].transpose(-1, -2) - lse[:, qq, None]) * mask
            ds = p * (dao[:, qq] @ v[:, kk].transpose(-1, -2) - D[:, qq, None])
            dq[:, qq] += (ds @ k[:, kk]) * 0.125
    return ao, lse, dq, dk, dv


def qkv_bias(b: torch.Tensor, rounding: bool) -> torch.Tensor:
    """The mode adds nothing to the k third of a qkv bias gradient (identically zero in exact arithmetic: a softmax row ignores a
    common shift of its logits; under the roundings above it would be the residue of sum_k bf16(dS) alone): the k third of
    the bias is a constant of the rounded step.  Unrounded, autograd's own 1e-17 stays."""
    if not rounding:
        return b
    n = b.shape[0] // 3
    return torch.cat([b[:n], b[n:2 * n].detach(), b[2 * n:]])


def forward_features(sd: dict, img: torch.Tensor, patch: int, stride: int, rounding: bool = True, eps: float = 1e-6):
    """tests/s3_bf16_reference.py `forward_features` with the attention of this module: MixedLinear layers and FlashAttention
    round together (`rounding`), as gemm_mode 3 does."""
    dim = sd["pos_embed"].shape[-1]
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    heads = dim // 64
    lin = lambda h, name: MP.MixedLinear.apply(h, sd[name + ".weight"], sd[name + ".bias"], rounding)  # noqa: E731
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
        qkv = MP.MixedLinear.apply(h, sd[p + "attn.qkv.weight"], qkv_bias(sd[p + "attn.qkv.bias"], rounding), rounding)
        q, k, v = qkv.reshape(B, -1, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)
        a = attention(q, k, v, rounding)
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
