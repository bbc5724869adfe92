"""CPU: the host side of the stage-3 step's opt-in bf16 mode -- the comparator of tests/s3_bf16_reference.py against plain
float64 autograd, the new C ABI (symbols, signatures, the refusals that need no device) and the driver's `--dtype`."""
import ctypes as C

import pytest
import torch

from tests import s3_bf16_reference as MP
from tests import s3_reference as REF


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def problem(dim, depth, img, batch, n_reg=0, seed=0):
    from dvt_amd.vit import random_state_dict
    g = (img - 14) // 14 + 1
    sd = random_state_dict(dim, depth, 14, (0 if n_reg else 1) + g * g, seed=seed, well_conditioned=True, n_reg=n_reg)
    gen = torch.Generator().manual_seed(seed + 1)
    return sd, torch.randn(batch, 3, img, img, generator=gen), torch.randn(batch, g, g, dim, generator=gen)


@pytest.mark.parametrize("n_reg", [0, 4])
def test_comparator_without_rounding_is_float64_autograd(n_reg):
    """The restated forward and the hand-written backward of MixedLinear, rounding off, against oracle/vit.py + autograd."""
    sd, x, t = problem(128, 2, 42, 2, n_reg)
    want_f, want_l, want_g = REF.step(sd, x, t)
    got_f, got_l, got_g = MP.step(sd, x, t, rounding=False)
    assert rel(got_f, want_f) <= 1e-12
    assert all(abs(a - b) <= 1e-12 * max(1.0, abs(b)) for a, b in zip(got_l, want_l))
    assert set(got_g) == set(want_g)
    errs = {k: rel(got_g[k], want_g[k]) for k in want_g}
    assert all(v <= 1e-12 for v in errs.values()), errs


def test_comparator_rounds_what_the_mode_rounds():
    """Rounding on: the step moves by about the bf16 rounding unit, and a lone layer shows which products are rounded: the
    forward and the data gradient see bf16 operands, the weight and bias gradients the unrounded ones."""
    sd, x, t = problem(128, 1, 42, 2)
    _, want_l, want_g = REF.step(sd, x, t)
    _, got_l, got_g = MP.step(sd, x, t)
    errs = {k: rel(got_g[k], want_g[k]) for k in want_g}
    assert 1e-4 < max(errs.values()) < 1e-1, errs  # 2^-9 per operand: far above float64, far below a wrong product
    assert abs(got_l[0] - want_l[0]) < 1e-2 * abs(want_l[0])
    g = torch.Generator().manual_seed(3)
    xx = torch.randn(5, 8, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(6, 8, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(6, generator=g, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(5, 6, generator=g, dtype=torch.float64)
    y = MP.MixedLinear.apply(xx, w, b, True)
    y.backward(dy)
    assert torch.equal(y.detach(), MP.bf16(xx.detach()) @ MP.bf16(w.detach()).t() + b.detach())
    assert torch.equal(xx.grad, MP.bf16(dy) @ MP.bf16(w.detach()))
    assert torch.equal(w.grad, dy.t() @ xx.detach()) and torch.equal(b.grad, dy.sum(0))
    # bf16(.) is round to nearest even on fp32 values: 1 + 2^-8 is a tie and goes to the even mantissa, 1 + 3 * 2^-8 up
    assert MP.bf16(torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], dtype=torch.float64)).tolist() == [1.0, 1 + 2.0 ** -6]


def test_abi_symbols_and_refusals(built_lib):
    """The new entry points exist with the declared signatures; an unknown gemm_mode, a negative grid and a workspace below
    the mode's size are refused with DVT_E_BADARG before anything is launched or any pointer is touched (no device here: the
    pointers below are made up)."""
    from dvt_amd import _lib, s3
    L = built_lib
    P, I, L64 = C.c_void_p, C.c_int, C.c_int64
    cfgp = C.POINTER(s3.VitConfig)
    want = {"dvt_s3_workspace_bytes_mp": (L64, [cfgp, I, I, I]),
            "dvt_s3_train_slice_pos_mp": (I, [cfgp, I, P, P, I, P, P, P, P, P, I, I, P, L64, P, P]),
            "dvt_s3_cast_bf16": (I, [P, P, L64, I, P]),
            "dvt_s3_cast_bf16_t": (I, [P, P, I, I, P])}
    for name, (res, args) in want.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    cfg = s3.make_config(384, 2, 14, 14, 98, 98)
    f32 = L.dvt_s3_workspace_bytes(C.byref(cfg), 2)
    assert L.dvt_s3_workspace_bytes_mp(C.byref(cfg), 2, 0, 0) == f32  # mode 0 is the fp32 step, byte for byte
    assert L.dvt_s3_workspace_bytes_mp(C.byref(cfg), 2, 7, 0) == L.dvt_s3_workspace_bytes_pos(C.byref(cfg), 2, 7) == f32
    assert L.dvt_s3_workspace_bytes_mp(C.byref(cfg), 2, 5, 0) == L.dvt_s3_workspace_bytes_pos(C.byref(cfg), 2, 5)
    mp = L.dvt_s3_workspace_bytes_mp(C.byref(cfg), 2, 0, 1)
    # the mode's share: two bf16 copies of the four weights of each block, one A scratch of R x max(mlp, 3 dim) bf16
    share = 2 * (2 * 2 * (3 * 384 * 384 + 384 * 384 + 2 * 1536 * 384)) + 2 * 256 * 1536
    assert f32 + share <= mp <= f32 + share + 256 * (2 * 4 * 2 + 1)  # (every piece starts on a 256-byte boundary)
    for bad_mode in (2, -1):
        assert L.dvt_s3_workspace_bytes_mp(C.byref(cfg), 2, 0, bad_mode) == -1
    assert L.dvt_s3_workspace_bytes_mp(C.byref(cfg), 2, -1, 1) == -1
    fake = 0x10000  # never dereferenced: every call below is refused first

    def slice_mp(mode, g0, work_bytes):
        return L.dvt_s3_train_slice_pos_mp(C.byref(cfg), g0, None, None, mode, fake, fake, fake, fake, None, 2, 2, fake,
                                           work_bytes, fake, None)
    assert slice_mp(2, 0, mp) == -1 and slice_mp(-1, 0, mp) == -1 and slice_mp(1, -1, mp) == -1
    assert slice_mp(1, 0, mp - 1) == -1 and slice_mp(1, 0, f32) == -1  # the fp32 mode's workspace is too small for mode 1
    assert slice_mp(0, 0, f32 - 1) == -1
    assert slice_mp(1, 5, mp) == -1  # a table at another grid needs its two interpolation tables
    assert L.dvt_s3_train_slice_pos_mp(C.byref(cfg), 0, None, None, 1, None, fake, fake, fake, None, 2, 2, fake, mp, fake,
                                       None) == -1  # null params
    assert L.dvt_s3_train_slice_pos_mp(C.byref(cfg), 0, None, None, 1, fake + 4, fake, fake, fake, None, 2, 2, fake, mp, fake,
                                       None) == -1  # params off the 16-byte grid
    # the casts: shapes and alignment
    assert L.dvt_s3_cast_bf16(fake, fake, 4, 6, None) == -1 and L.dvt_s3_cast_bf16(None, fake, 4, 8, None) == -1
    assert L.dvt_s3_cast_bf16(fake + 8, fake, 4, 8, None) == -1 and L.dvt_s3_cast_bf16(fake, fake, 0, 8, None) == -1
    assert L.dvt_s3_cast_bf16_t(fake, fake, 96, 64, None) == -1 and L.dvt_s3_cast_bf16_t(fake, fake, 64, 32, None) == -1
    assert L.dvt_s3_cast_bf16_t(fake, None, 64, 64, None) == -1 and L.dvt_s3_cast_bf16_t(fake, fake + 2, 64, 64, None) == -1
    with pytest.raises(_lib.DvtError, match="dtype"):
        s3.Stage3Engine(cfg, torch.device("cuda"), dtype="float16")  # (refused before the device is looked at)


def test_cli_dtype():
    from dvt_amd import stage3
    base = ["--denoiser_ckpt", "x.pth"]
    assert stage3.get_args(base).dtype == "float32"
    assert stage3.get_args(base + ["--dtype", "bfloat16"]).dtype == "bfloat16"
    assert stage3.get_args(base + ["--dtype", "float32"]).dtype == "float32"
    for bad in ("float16", "bf16", "fp32"):
        with pytest.raises(SystemExit):
            stage3.get_args(base + ["--dtype", bad])
    from dvt_amd import s3
    assert s3.GEMM_MODES == {"float32": 0, "bfloat16": 1}
