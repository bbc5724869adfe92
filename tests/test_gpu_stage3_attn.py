"""GPU: the bf16 flash attention kernels of the stage-3 step (csrc/dvt_s3_attn.hip) through `dvt_s3_attn_fwd` /
`dvt_s3_attn_bwd`, batch 2, heads 2, on the key census of tests/attention_reference.py (probe V, planted pad K / V rows).

Forward, per element and relative (the census' V makes every output a sum of positive terms): the tolerance is the one
tests/attention_reference.py derives for the log2q kernel less the output's own bf16 rounding, since `ao` is fp32 here --
    e = rel_bound(ref, "log2q", T) - BF16 = BF16 + 4 e32,   tol = e ref + FLOOR
with its terms `BF16` (the one rounding of P for P v), `e32` (2 (dz + 4 U) + 2 (T + 8) U with dz = 67 U (M + A): the logit chain,
exp2, the fp32 sums) and `FLOOR`; the reference is float64 attention of the operands the kernel is handed (`operands`, q
pre-scaled and rounded once).  2^lse against the float64 row sum of e^z, relative, within that same e32: the logit error dz
enters each term once, the sum is (T + 8) U, and the rounding of lse = m + log2(l) itself is U |lse| ln 2 <= U M, inside dz.

Backward, per (image, head) tensor: relative-L2 distance from float64 autograd of softmax(q k^T / 8) v on the unrounded inputs
at most 2 x the distance of the comparator tests/s3_attn_reference.py, which rounds what the kernels round and accumulates
exactly (the convention of tests/test_gpu_stage3_bf16.py)."""
import ctypes as C
import functools

import pytest
import torch

from tests import attention_reference as AR
from tests import s3_attn_reference as ATT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADS = 2
# (T, Tp): a single partial key tile; the step tests' shape; two query blocks with 17 valid keys in the last tile; one key
# past a tile edge; valid keys end on a tile edge
SHAPES = [(17, 128), (50, 128), (145, 256), (257, 384), (320, 384)]
FWD_PATTERNS = [("random", "stairs"), ("spikes8.5", "random")]
BWD_PATTERNS = ("random", "spikes8.5")  # spikes: one dominant key per row, P near 1 and dP - D near 0


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def qkv_rows(inp):
    """q, k, v [B, S, H, 64] -> fp32 [B * S, 3 * 64 * H] as the qkv GEMM writes it."""
    B, S = inp["q"].shape[:2]
    return torch.cat([inp[n].reshape(B * S, -1) for n in ("q", "k", "v")], dim=1).contiguous()


@functools.lru_cache(maxsize=None)
def forward_run(T, Tp, patterns):
    """One forward on the census inputs: (ao [B, S, H, 64], lse [B, H, S], the kept operands, ao as the kernel wrote it)."""
    from dvt_amd import s3
    inp = AR.census_inputs(T, Tp, HEADS, patterns)
    B = len(patterns)
    ao, lse, qkvb = s3.attn_fwd(qkv_rows(inp).to(DEV), B, HEADS, T)
    torch.cuda.synchronize()
    return ao.cpu().reshape(B, Tp, HEADS, 64), lse.cpu().reshape(B, HEADS, Tp), qkvb, ao


@pytest.mark.parametrize("patterns", FWD_PATTERNS, ids="+".join)
@pytest.mark.parametrize("T,Tp", SHAPES)
def test_forward_per_key(T, Tp, patterns):
    c = AR.case("log2q", T, Tp, HEADS, patterns)
    ao, lse, qkvb, _ = forward_run(T, Tp, patterns)
    # the kept operands are the handed ones, bit for bit: q pre-scaled and rounded once, k, v rounded once
    for i, want in enumerate(c["handed"]):
        assert torch.equal(qkvb[i].cpu().view(torch.int16), want.permute(0, 2, 1, 3).reshape(-1, Tp, 64).contiguous().view(torch.int16))
    ref = c["ref"]
    e = AR.rel_bound(ref, "log2q", T) - AR.BF16
    e32 = (AR.rel_bound(ref, "log2q", T) - 2 * AR.BF16) / 4
    tol = e * ref["out"] + AR.FLOOR
    ratio = ((ao.double() - ref["out"]).abs() / tol)[:, :T].nan_to_num(nan=float("inf")).amax(dim=(1, 2, 3))
    rowsum = torch.exp(ref["z"]).sum(-1)[:, :, :T]                                   # [B, H, T]
    lse_err = (torch.exp2(lse.double()[:, :, :T]) - rowsum).abs() / rowsum
    lse_ratio = (lse_err / e32[..., 0].permute(0, 2, 1)[:, :, :T]).nan_to_num(nan=float("inf")).amax(dim=(1, 2))
    print(f"s3 attention forward T={T} Tp={Tp} {patterns}: worst |ao - f64| / tol {ratio.tolist()}, worst lse error / e32 "
          f"{lse_ratio.tolist()}")
    assert (ratio <= 1).all(), ratio
    assert (lse_ratio <= 1).all(), lse_ratio
    assert not ao[:, T:].any()  # pad rows: exactly zero


@functools.lru_cache(maxsize=None)
def backward_run(T, Tp):
    """(inputs, dao [B, S, H, 64], dqkv of the kernels as (dq, dk, dv) [B, S, H, 64], the device tensors of the run)."""
    from dvt_amd import s3
    inp = AR.census_inputs(T, Tp, HEADS, BWD_PATTERNS)
    B = len(BWD_PATTERNS)
    dao = torch.randn(B, Tp, HEADS, 64, generator=torch.Generator().manual_seed(T))
    _, lse, qkvb, ao = forward_run(T, Tp, BWD_PATTERNS)
    dao_d = dao.reshape(B * Tp, -1).to(DEV)
    dqkv = s3.attn_bwd(qkvb, ao, dao_d, lse.to(DEV).reshape(B * HEADS, Tp), B, HEADS, T)
    torch.cuda.synchronize()
    return inp, dao, tuple(t.reshape(B, Tp, HEADS, 64) for t in dqkv.cpu().chunk(3, dim=1)), (qkvb, ao, dao_d, lse.to(DEV))


@pytest.mark.parametrize("T,Tp", SHAPES)
def test_backward_vs_float64(T, Tp):
    inp, dao, got, _ = backward_run(T, Tp)

    def grads(fn):
        leaves = [inp[n][:, :T].double().permute(0, 2, 1, 3).clone().requires_grad_(True) for n in ("q", "k", "v")]
        fn(*leaves).backward(dao[:, :T].double().permute(0, 2, 1, 3))
        return [t.grad for t in leaves]                                             # [B, H, T, 64]
    f64 = grads(lambda q, k, v: torch.softmax(q @ k.transpose(-1, -2) / 8, -1) @ v)
    cmp = grads(ATT.attention)
    worst = 0.0
    for name, g, want, yard in zip(("dq", "dk", "dv"), got, f64, cmp):
        assert not g[:, T:].any(), name  # rows t >= T: exactly zero, whatever the planted pad rows hold
        for b, pat in enumerate(BWD_PATTERNS):
            for h in range(HEADS):
                d, y = rel(g[b, :T, h], want[b, h]), rel(yard[b, h], want[b, h])
                worst = max(worst, d / y)
                print(f"  T={T} {pat} head {h} {name}: kernels {d:.3e}, comparator {y:.3e}, ratio {d / y:.3f}")
                assert d <= 2 * y, (name, pat, h, d, y)
    print(f"s3 attention backward T={T} Tp={Tp}: worst ratio to the comparator {worst:.3f}")


@pytest.mark.parametrize("T,Tp", [(50, 128), (145, 256)])
def test_same_bits_on_every_run(T, Tp):
    from dvt_amd import s3
    inp = AR.census_inputs(T, Tp, HEADS, BWD_PATTERNS)
    _, _, first, (qkvb, ao, dao_d, lse) = backward_run(T, Tp)
    B = len(BWD_PATTERNS)
    ao2, lse2, qkvb2 = s3.attn_fwd(qkv_rows(inp).to(DEV), B, HEADS, T)
    dqkv2 = s3.attn_bwd(qkvb2, ao2, dao_d, lse2, B, HEADS, T)
    assert torch.equal(ao2, ao) and torch.equal(lse2.reshape(-1), lse.reshape(-1)) and torch.equal(qkvb2, qkvb)
    again = tuple(t.reshape(B, Tp, HEADS, 64) for t in dqkv2.cpu().chunk(3, dim=1))
    assert all(torch.equal(a, b) for a, b in zip(again, first))


def test_argument_checks():
    """DVT_E_BADARG with nothing launched: the outputs keep their fill."""
    from dvt_amd import _lib
    L = _lib.lib()
    B, Tp, T = 2, 128, 50
    qkv = torch.randn(B * Tp, 3 * 64 * HEADS, device=DEV)
    qkvb = torch.zeros(3, B * HEADS, Tp, 64, device=DEV, dtype=torch.bfloat16)
    ao = torch.full((B * Tp, 64 * HEADS), 7.0, device=DEV)
    lse = torch.full((B * HEADS, Tp), 7.0, device=DEV)
    dqkv = torch.full((B * Tp, 3 * 64 * HEADS), 7.0, device=DEV)
    p = _lib.ptr

    def fwd(qkv_=p(qkv), qkvb_=p(qkvb), ao_=p(ao), lse_=p(lse), T_=T, Tp_=Tp):
        return L.dvt_s3_attn_fwd(qkv_, qkvb_, ao_, lse_, B, HEADS, T_, Tp_, _lib.stream())

    def bwd(qkvb_=p(qkvb), ao_=p(ao), dao_=p(ao), lse_=p(lse), D_=p(lse), dqkv_=p(dqkv), T_=T, Tp_=Tp):
        return L.dvt_s3_attn_bwd(qkvb_, ao_, dao_, lse_, D_, dqkv_, B, HEADS, T_, Tp_, _lib.stream())
    for kw in (dict(qkv_=None), dict(qkvb_=None), dict(ao_=None), dict(lse_=None), dict(Tp_=64), dict(Tp_=192), dict(T_=Tp + 1),
               dict(T_=0), dict(T_=-1)):
        assert fwd(**kw) == -1, kw
    for kw in (dict(qkvb_=None), dict(ao_=None), dict(dao_=None), dict(lse_=None), dict(D_=None), dict(dqkv_=None),
               dict(Tp_=192), dict(T_=Tp + 1), dict(T_=0)):
        assert bwd(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (ao == 7).all() and (lse == 7).all() and (dqkv == 7).all() and not qkvb.any()
    assert C.c_int(fwd()).value == 0  # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert not (ao == 7).any()
