"""CPU: the host side of the stage-3 step's bf16 weight gradients (gemm_modes 5 and 7) -- the comparator of
tests/s3_wgrad_reference.py against plain float64 autograd and against the products it claims to round, the C ABI's symbols,
workspace sizes and refusals that need no device, and the Python interface and driver flags."""
import ctypes as C

import pytest
import torch

from tests import s3_bf16_reference as MP
from tests import s3_reference as REF
from tests import s3_wgrad_reference as WG
from tests.test_stage3_bf16_cpu import problem, rel


@pytest.mark.parametrize("attention", [False, True])
@pytest.mark.parametrize("n_reg", [0, 4])
def test_comparator_without_rounding_is_float64_autograd(n_reg, attention):
    """The restated forward with WgradLinear's hand-written backward, rounding off, against oracle/vit.py + autograd."""
    sd, x, t = problem(128, 2, 42, 2, n_reg)
    want_f, want_l, want_g = REF.step(sd, x, t)
    got_f, got_l, got_g = WG.step(sd, x, t, rounding=False, attention=attention)
    assert rel(got_f, want_f) <= 1e-12
    assert all(abs(a - b) <= 1e-12 * max(1.0, abs(b)) for a, b in zip(got_l, want_l))
    assert set(got_g) == set(want_g)
    errs = {k: rel(got_g[k], want_g[k]) for k in want_g}
    assert all(v <= 1e-12 for v in errs.values()), errs


def test_comparator_rounds_what_the_mode_rounds():
    """A lone layer with rounding on: the forward and data gradient are MixedLinear's, w.grad is exactly bf16(dy)^T bf16(x) and
    b.grad exactly colsum(dy) of the unrounded dy."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 40, 24, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(16, 24, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(16, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(3, 40, 16, generator=g, dtype=torch.float64)
    y = WG.WgradLinear.apply(x, w, b, True)
    y.backward(dy)
    r = MP.bf16
    assert torch.equal(y.detach(), r(x.detach()) @ r(w.detach()).t() + b.detach())
    assert torch.equal(x.grad, r(dy) @ r(w.detach()))
    assert torch.equal(w.grad, r(dy).reshape(-1, 16).t() @ r(x.detach()).reshape(-1, 24))
    assert torch.equal(b.grad, dy.reshape(-1, 16).sum(0))
    assert not torch.equal(w.grad, dy.reshape(-1, 16).t() @ x.detach().reshape(-1, 24))  # (the rounding is visible)
    # the same layer as MixedLinear: everything but w.grad agrees
    x2, w2, b2 = (v.detach().clone().requires_grad_() for v in (x, w, b))
    MP.MixedLinear.apply(x2, w2, b2, True).backward(dy)
    assert torch.equal(x2.grad, x.grad) and torch.equal(b2.grad, b.grad) and not torch.equal(w2.grad, w.grad)


def test_python_refusals_and_flags():
    """`weight_grad="bfloat16"` needs `dtype="bfloat16"`; an unknown value is refused by name -- both before the device is looked
    at -- and the driver applies the same rule to `--weight_grad`."""
    from dvt_amd import _lib, s3, stage3
    cfg = s3.make_config(384, 2, 14, 14, 98, 98)
    with pytest.raises(_lib.DvtError, match='weight_grad="bfloat16".*dtype="bfloat16"'):
        s3.Stage3Engine(cfg, torch.device("cuda"), dtype="float32", weight_grad="bfloat16")
    with pytest.raises(_lib.DvtError, match="weight_grad='float16'"):
        s3.Stage3Engine(cfg, torch.device("cuda"), dtype="bfloat16", weight_grad="float16")
    assert s3.WEIGHT_GRAD_MODES == {"float32": 0, "bfloat16": 4}
    assert s3.GEMM_MODES["bfloat16"] | s3.WEIGHT_GRAD_MODES["bfloat16"] == 5
    assert s3.GEMM_MODES["bfloat16"] | s3.ATTENTION_MODES["bfloat16"] | s3.WEIGHT_GRAD_MODES["bfloat16"] == 7
    base = ["--denoiser_ckpt", "x.pth"]
    assert stage3.get_args(base).weight_grad == "float32"
    assert stage3.get_args(base + ["--dtype", "bfloat16", "--weight_grad", "bfloat16"]).weight_grad == "bfloat16"
    a = stage3.get_args(base + ["--dtype", "bfloat16", "--attention", "bfloat16", "--weight_grad", "bfloat16"])
    assert (a.dtype, a.attention, a.weight_grad) == ("bfloat16",) * 3
    with pytest.raises(SystemExit, match="--weight_grad bfloat16 needs --dtype bfloat16"):
        stage3.get_args(base + ["--weight_grad", "bfloat16"])
    with pytest.raises(SystemExit):
        stage3.get_args(base + ["--dtype", "bfloat16", "--weight_grad", "bf16"])


def up256(b):
    return (b + 255) // 256 * 256


def splits_rule(R, n, k):
    """The rule stated in include/dvt_stage3.h: S = min(ceil(1024 / tiles), R / 256), at least 1."""
    tiles = (n // 128) * (k // 128)
    return max(1, min(-(-1024 // tiles), R // 256))


def test_abi_workspace_and_refusals(built_lib):
    """ViT-S at 98 x 98, batch 2 (R = 256).  Modes 5 and 7 need mode 1's resp. 3's workspace plus the documented share behind it:
    the layer input's row cast (2 max(mlp, dim) bytes per row) and the largest layer's partial tiles (4 S n k + 4 Sb n), each
    piece in whole 256-byte units; 4, 6, 8 and -1 stay refused; a mode-5 slice on mode 1's workspace is refused; every refusal of
    dvt_s3_wgrad_bf16 (no device here: the pointers are made up and never dereferenced)."""
    from dvt_amd import s3
    L = built_lib
    P, I, L64 = C.c_void_p, C.c_int, C.c_int64
    want = {"dvt_s3_wgrad_bf16_scratch_bytes": (L64, [L64, I, I, I]),
            "dvt_s3_wgrad_bf16": (I, [P, P, P, P, P, L64, L64, I, I, I, I, P])}
    for name, (res, args) in want.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    cfg = s3.make_config(384, 2, 14, 14, 98, 98)
    batch, dim, mlp = 2, 384, 1536
    R = batch * cfg.s_pad
    assert (cfg.s_pad, cfg.mlp_dim) == (128, mlp)
    layers = [(3 * dim, dim), (dim, dim), (mlp, dim), (dim, mlp)]
    sb = max(1, min(128, R // 1024))
    share = up256(2 * R * max(mlp, dim)) + max(up256(4 * splits_rule(R, n, k) * n * k) + up256(4 * sb * n) for n, k in layers)
    sizes = {m: L.dvt_s3_workspace_bytes_mp(C.byref(cfg), batch, 0, m) for m in (1, 3, 5, 7)}
    assert sizes[5] == sizes[1] + share and sizes[7] == sizes[3] + share, (sizes, share)
    for bad_mode in (2, 4, 6, 8, -1):
        assert L.dvt_s3_workspace_bytes_mp(C.byref(cfg), batch, 0, bad_mode) == -1
    fake = 0x10000

    def slice_mp(mode, work_bytes, params=fake):
        return L.dvt_s3_train_slice_pos_mp(C.byref(cfg), 0, None, None, mode, params, fake, fake, fake, None, batch, batch, fake,
                                           work_bytes, fake, None)
    for bad_mode in (2, 4, 6, 8, -1):
        assert slice_mp(bad_mode, sizes[1]) == -1
    assert slice_mp(5, sizes[1]) == -1 and slice_mp(5, sizes[5] - 1) == -1 and slice_mp(7, sizes[3]) == -1
    assert slice_mp(5, sizes[5], fake + 4) == -1 and slice_mp(7, sizes[7], None) == -1
    # the exported kernel: sizes, then every refusal
    nb = L.dvt_s3_wgrad_bf16_scratch_bytes
    assert nb(1408, 128, 384, 3) == up256(2 * 1408 * 128) + up256(2 * 1408 * 384) + up256(4 * 3 * 128 * 384) + up256(4 * 128)
    assert nb(1408, 128, 384, 0) == nb(1408, 128, 384, splits_rule(1408, 128, 384)) and splits_rule(1408, 128, 384) == 5
    assert nb(256, 128, 128, 1000) == nb(256, 128, 128, 4)  # clamped to the R / 64 row steps
    assert nb(90112, 768, 768, 0) == nb(90112, 768, 768, 29) and nb(90112, 3072, 768, 0) == nb(90112, 3072, 768, 8)
    for bad in ((0, 128, 128, 0), (192, 128, 128, 0), (128, 64, 128, 0), (128, 128, 192, 0), (128, 128, 128, -1), (-128, 128, 128, 0)):
        assert nb(*bad) == -1, bad
    ok = nb(256, 128, 384, 0)

    def run(dy=fake, x=fake, dw=fake, db=fake, scratch=fake, sbytes=ok, R=256, n=128, k=384, splits=0):
        return L.dvt_s3_wgrad_bf16(dy, x, dw, db, scratch, sbytes, R, n, k, splits, 0, None)
    for kw in (dict(dy=None), dict(x=None), dict(dw=None), dict(db=None), dict(scratch=None), dict(dy=fake + 4), dict(x=fake + 8),
               dict(dw=fake + 4), dict(db=fake + 4), dict(scratch=fake + 2), dict(sbytes=ok - 1), dict(sbytes=0), dict(splits=-1),
               dict(R=0), dict(R=192), dict(R=-256), dict(n=64), dict(n=192), dict(n=0), dict(k=0), dict(k=448),
               dict(splits=4, sbytes=nb(256, 128, 384, 4) - 1)):
        assert run(**kw) == -1, kw
