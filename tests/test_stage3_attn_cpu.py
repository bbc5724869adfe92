"""CPU: the host side of the stage-3 step's bf16 flash attention (gemm_mode 3) -- the comparator of
tests/s3_attn_reference.py against plain float64 autograd, the recompute identity and the two-pass gradient split in float64,
the refusals of the Python interface and of the C ABI that need no device, and the workspace the mode gives back."""
import ctypes as C

import pytest
import torch

from tests import s3_attn_reference as ATT
from tests import s3_reference as REF
from tests.test_stage3_bf16_cpu import problem, rel


@pytest.mark.parametrize("n_reg", [0, 4])
def test_comparator_without_rounding_is_float64_autograd(n_reg):
    """The restated forward with FlashAttention's hand-written backward, rounding off, against oracle/vit.py + autograd."""
    sd, x, t = problem(128, 2, 42, 2, n_reg)
    want_f, want_l, want_g = REF.step(sd, x, t)
    got_f, got_l, got_g = ATT.step(sd, x, t, rounding=False)
    assert rel(got_f, want_f) <= 1e-12
    assert all(abs(a - b) <= 1e-12 * max(1.0, abs(b)) for a, b in zip(got_l, want_l))
    assert set(got_g) == set(want_g)
    errs = {k: rel(got_g[k], want_g[k]) for k in want_g}
    assert all(v <= 1e-12 for v in errs.values()), errs


def test_comparator_rounds_what_the_mode_rounds():
    """Rounding on, a lone attention of one key tile: the forward is bf16(2^(s - max)) bf16(v) / sum of the rounded,
    pre-scaled q and rounded k; lse and D are not rounded; the three gradients are the products the module docstring lists,
    term by term.  With 40 keys (two tiles) the first tile's P is rounded against the first tile's maximum."""
    g = torch.Generator().manual_seed(5)
    q, k, v, dao = (torch.randn(2, 9, 64, generator=g, dtype=torch.float64) for _ in range(4))
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    ao = ATT.attention(ql, kl, vl)
    ao.backward(dao)
    b = ATT.MP.bf16
    qs, kb, vb = b(q * ATT.Q_PRESCALE), b(k), b(v)
    s = qs @ kb.transpose(-1, -2)
    lse = torch.log2(torch.exp2(s).sum(-1, keepdim=True))
    p = torch.exp2(s - lse)
    e = torch.exp2(s - s.amax(-1, keepdim=True))
    assert rel(ao, b(e) @ vb / e.sum(-1, keepdim=True)) <= 1e-14
    D = (dao * ao.detach()).sum(-1, keepdim=True)
    ds = b(p * (b(dao) @ vb.transpose(-1, -2) - D))
    assert rel(vl.grad, b(p).transpose(-1, -2) @ b(dao)) <= 1e-13
    assert rel(ql.grad, ds @ kb / 8) <= 1e-13 and rel(kl.grad, ds.transpose(-1, -2) @ qs * ATT.LN2) <= 1e-13
    # and it moves the result by about the bf16 unit: far above float64, far below a wrong product
    ao64 = torch.softmax(q @ k.transpose(-1, -2) / 8, -1) @ v
    assert 1e-4 < rel(ao, ao64) < 3e-2
    q, k, v = (torch.randn(1, 40, 64, generator=g, dtype=torch.float64) for _ in range(3))
    qs, kb, vb = b(q * ATT.Q_PRESCALE), b(k), b(v)
    s = qs @ kb.transpose(-1, -2)
    m1, m = s[..., :32].amax(-1, keepdim=True), s.amax(-1, keepdim=True)
    num = torch.exp2(m1 - m) * (b(torch.exp2(s[..., :32] - m1)) @ vb[:, :32]) + b(torch.exp2(s[..., 32:] - m)) @ vb[:, 32:]
    ao, lse = ATT.forward_lse(q, k, v)
    assert rel(ao, num / torch.exp2(s - m).sum(-1, keepdim=True)) <= 1e-14
    assert rel(lse, torch.log2(torch.exp2(s).sum(-1))) <= 1e-14


@pytest.mark.parametrize("n_valid,s_pad", [(17, 128), (145, 256)])
def test_recompute_identity_and_gradient_split(n_valid, s_pad):
    """float64, 2 heads, pad rows filled with large values that must not leak: 2^(s - lse) IS the softmax, and the two passes
    of the backward (key blocks sweeping query tiles for dk / dv, query blocks sweeping key tiles for dq, each recomputing P
    from lse) give autograd's gradients of softmax(q k^T / 8) v to 1e-12; rows >= T of every output are exactly zero."""
    g = torch.Generator().manual_seed(n_valid)
    q, k, v, dao = (torch.randn(2, s_pad, 64, generator=g, dtype=torch.float64) for _ in range(4))
    k[:, n_valid:] = 50.0
    v[:, n_valid:] = 2.0 ** 14
    T = n_valid
    ql, kl, vl = (t[:, :T].clone().requires_grad_(True) for t in (q, k, v))
    p_ref = torch.softmax(ql @ kl.transpose(-1, -2) / 8, -1)
    ao_ref = p_ref @ vl
    ao_ref.backward(dao[:, :T])
    ao, lse, dq, dk, dv = ATT.tiled_backward(q, k, v, dao, T)
    s = (q[:, :T] * ATT.Q_PRESCALE) @ k[:, :T].transpose(-1, -2)
    assert rel(torch.exp2(s - lse[:, :T, None]), p_ref) <= 1e-12
    assert rel(ao[:, :T], ao_ref) <= 1e-12
    for got, want in ((dq, ql.grad), (dk, kl.grad), (dv, vl.grad)):
        assert rel(got[:, :T], want) <= 1e-12
        assert not got[:, T:].any()
    assert not ao[:, T:].any()
    # the comparator's backward without rounding is the same gradient
    q2, k2, v2 = (t[:, :T].clone().requires_grad_(True) for t in (q, k, v))
    ATT.attention(q2, k2, v2, rounding=False).backward(dao[:, :T])
    assert max(rel(q2.grad, ql.grad), rel(k2.grad, kl.grad), rel(v2.grad, vl.grad)) <= 1e-12


def test_python_refusals():
    """`attention="bfloat16"` needs `dtype="bfloat16"`; an unknown value is refused by name -- both before the device is looked
    at -- and the driver applies the same rule to `--attention`."""
    from dvt_amd import _lib, s3, stage3
    cfg = s3.make_config(384, 2, 14, 14, 98, 98)
    with pytest.raises(_lib.DvtError, match='attention="bfloat16".*dtype="bfloat16"'):
        s3.Stage3Engine(cfg, torch.device("cuda"), dtype="float32", attention="bfloat16")
    with pytest.raises(_lib.DvtError, match="attention='float16'"):
        s3.Stage3Engine(cfg, torch.device("cuda"), dtype="bfloat16", attention="float16")
    assert s3.GEMM_MODES["bfloat16"] | s3.ATTENTION_MODES["bfloat16"] == 3 and s3.ATTENTION_MODES["float32"] == 0
    base = ["--denoiser_ckpt", "x.pth"]
    assert stage3.get_args(base).attention == "float32"
    assert stage3.get_args(base + ["--dtype", "bfloat16", "--attention", "bfloat16"]).attention == "bfloat16"
    assert stage3.get_args(base + ["--dtype", "bfloat16"]).attention == "float32"
    with pytest.raises(SystemExit, match="--attention bfloat16 needs --dtype bfloat16"):
        stage3.get_args(base + ["--attention", "bfloat16"])
    with pytest.raises(SystemExit):
        stage3.get_args(base + ["--dtype", "bfloat16", "--attention", "bf16"])


def test_abi_workspace_and_refusals(built_lib):
    """ViT-S at 98 x 98, batch 2.  The attention mode (gemm_mode 3 = the bf16 GEMMs' bit | the attention's bit) needs at least
    depth * batch * heads * Tp * Tp * 4 bytes less workspace than mode 1 -- every block's P -- and what it adds is the bf16
    operands and lse of every block; the attention's bit without the GEMMs' (2) and any other value stay refused; a mode-3
    slice is refused on a workspace below its size and on unaligned parameters; the exported kernels refuse a null pointer,
    Tp % 128 != 0, T > Tp and T <= 0 (no device here: the pointers are made up and never dereferenced)."""
    from dvt_amd import s3
    L = built_lib
    P, I, L64 = C.c_void_p, C.c_int, C.c_int64
    want = {"dvt_s3_attn_operand_bytes": (L64, [I, I, I]),
            "dvt_s3_attn_fwd": (I, [P, P, P, P, I, I, I, I, P]),
            "dvt_s3_attn_bwd": (I, [P, P, P, P, P, P, I, I, I, I, P])}
    for name, (res, args) in want.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    cfg = s3.make_config(384, 2, 14, 14, 98, 98)
    depth, batch, heads, Tp, dim = 2, 2, 6, 128, 384
    assert (cfg.depth, cfg.heads, cfg.s_pad) == (depth, heads, Tp)
    m1 = L.dvt_s3_workspace_bytes_mp(C.byref(cfg), batch, 0, 1)
    m3 = L.dvt_s3_workspace_bytes_mp(C.byref(cfg), batch, 0, 3)
    assert 0 < m3 <= m1 - depth * batch * heads * Tp * Tp * 4
    # exactly: less P per block, the dP scratch and fp32 qkv per block; more bf16 operands and lse per block, and one
    # [3 dim] buffer for the qkv bias gradient's column sums
    R = batch * Tp
    less = (depth + 1) * batch * heads * Tp * Tp * 4 + depth * R * 3 * dim * 4
    more = depth * (R * 3 * dim * 2 + batch * heads * Tp * 4) + 3 * dim * 4
    assert m3 == m1 - less + more
    assert L.dvt_s3_attn_operand_bytes(batch, heads, Tp) == R * 3 * dim * 2
    for bad_mode in (2, 4, -1):
        assert L.dvt_s3_workspace_bytes_mp(C.byref(cfg), batch, 0, bad_mode) == -1
    fake = 0x10000

    def slice_mp(mode, work_bytes, params=fake):
        return L.dvt_s3_train_slice_pos_mp(C.byref(cfg), 0, None, None, mode, params, fake, fake, fake, None, batch, batch, fake,
                                           work_bytes, fake, None)
    assert slice_mp(2, m1) == -1 and slice_mp(4, m1) == -1
    assert slice_mp(3, m3 - 1) == -1 and slice_mp(3, m3, fake + 4) == -1 and slice_mp(3, m3, None) == -1
    fwd = lambda qkv=fake, qkvb=fake, ao=fake, lse=fake, T=50, tp=128: L.dvt_s3_attn_fwd(qkv, qkvb, ao, lse, 2, 2, T, tp, None)  # noqa: E731
    bwd = lambda qkvb=fake, ao=fake, dao=fake, lse=fake, D=fake, dqkv=fake, T=50, tp=128: L.dvt_s3_attn_bwd(  # noqa: E731
        qkvb, ao, dao, lse, D, dqkv, 2, 2, T, tp, None)
    for kw in (dict(qkv=None), dict(qkvb=None), dict(ao=None), dict(lse=None), dict(tp=192), dict(tp=64), dict(T=129), dict(T=0),
               dict(T=-3), dict(qkv=fake + 4)):
        assert fwd(**kw) == -1, kw
    for kw in (dict(qkvb=None), dict(ao=None), dict(dao=None), dict(lse=None), dict(D=None), dict(dqkv=None), dict(tp=192),
               dict(T=129), dict(T=0), dict(dqkv=fake + 8)):
        assert bwd(**kw) == -1, kw
