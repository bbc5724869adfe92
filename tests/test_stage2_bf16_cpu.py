"""CPU: the opt-in bf16 modes of the stage-2 training step (include/dvt_stage2.h `dvt_s2_workspace_bytes_mp` /
`dvt_s2_train_step_mp`, `Stage2Engine(dtype=, attention=, weight_grad=)`, `Denoiser(train_dtype=...)`, `python -m dvt_amd.stage2
--dtype / --attention / --weight_grad`) and the stage-3 trainer's `--teacher_dtype`: the comparator against the oracle, the
ABI's argument checks and workspace sizes, the defaults and the refusals of the Python layers.  No device is touched."""
import ctypes as C
import types

import pytest
import torch

from oracle import stage2 as O
from tests import s2_bf16_reference as S2REF


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---- the comparator ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks,enable_pe", [(1, True), (2, True), (1, False)])
@pytest.mark.parametrize("mode", S2REF.MODES)
def test_comparator_without_rounding_is_the_oracles_step(mode, blocks, enable_pe):
    """rounding=False: every mode of the comparator is the oracle's float64 autograd step -- pred, loss triple and every
    gradient to 1e-12 (relative L2; the loss terms relative).  That ties the restated forward, MixedLinear / WgradLinear and
    the hand-written flash-attention backward to oracle/stage2.py."""
    torch.manual_seed(3)
    ref = O.Denoiser(3, 5, 128, enable_pe, blocks)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    x, t = torch.randn(2, 3, 5, 128), torch.randn(2, 3, 5, 128)
    want_p, want_l, want_g = S2REF.oracle_step(ref, x, t)
    got_p, got_l, got_g = S2REF.step(ref.state_dict(), x, t, mode, rounding=False)
    assert rel(got_p, want_p) <= 1e-12
    assert all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(got_l, want_l)), (got_l, want_l)
    assert set(got_g) == set(want_g)
    worst = {k: rel(got_g[k], want_g[k]) for k in want_g}
    assert all(v <= 1e-12 for v in worst.values()), worst


def test_comparator_rounds_and_drops_the_k_bias():
    """With rounding the comparator leaves float64 autograd by about the bf16 unit; in modes 3 and 7 the k third of the qkv bias
    gradient is exactly zero, in modes 1 and 5 it is autograd's residue."""
    torch.manual_seed(4)
    ref = O.Denoiser(3, 5, 128, True, 1)
    x, t = torch.randn(2, 3, 5, 128), torch.randn(2, 3, 5, 128)
    _, _, want = S2REF.oracle_step(ref, x, t)
    for mode in S2REF.MODES:
        _, _, got = S2REF.step(ref.state_dict(), x, t, mode)
        d = rel(got["denoiser.attn.qkv.weight"], want["denoiser.attn.qkv.weight"])
        assert 1e-4 < d < 5e-2, (mode, d)
        kb = got["denoiser.attn.qkv.bias"][128:256]
        assert bool((kb == 0).all()) == bool(mode & 2), mode


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def cfg_for(dim, tokens, pad, blocks=1, mlp=None):
    from dvt_amd import s2
    c = s2.S2Config()
    c.dim, c.heads, c.mlp_dim = dim, dim // 64, 4 * dim if mlp is None else mlp
    c.tokens, c.tokens_pad, c.n_blocks, c.enable_pe, c.ln_eps = tokens, pad, blocks, 1, 1e-6
    return c


def test_abi_symbols_and_workspace(built_lib):
    from dvt_amd import s2  # noqa: F401  (registers the signatures)
    L = built_lib
    assert L.dvt_s2_workspace_bytes_mp.restype is C.c_int64 and callable(L.dvt_s2_train_step_mp)
    c = cfg_for(768, 1369, 1408)
    for bad in (-1, 2, 4, 6, 8):
        assert L.dvt_s2_workspace_bytes_mp(C.byref(c), 2, 1, bad) == -1, bad
    for training in (0, 1):
        assert L.dvt_s2_workspace_bytes_mp(C.byref(c), 2, training, 0) == L.dvt_s2_workspace_bytes(C.byref(c), 2, training) > 0
    for pad in (64, 192):  # whole 64-row tiles, which mode 0 takes, but no 128-row tiles
        small = cfg_for(384, 45, pad)
        assert L.dvt_s2_workspace_bytes_mp(C.byref(small), 2, 1, 0) > 0
        for mode in (1, 3, 5, 7):
            assert L.dvt_s2_workspace_bytes_mp(C.byref(small), 2, 1, mode) == -1, (pad, mode)
    assert L.dvt_s2_workspace_bytes_mp(C.byref(cfg_for(384, 45, 128, mlp=1472)), 2, 1, 1) == -1  # mlp_dim % 128
    assert L.dvt_s2_workspace_bytes_mp(C.byref(c), 2, 0, 1) == -1  # the modes train; inference has none
    w = {m: L.dvt_s2_workspace_bytes_mp(C.byref(c), 2, 1, m) for m in (0, 1, 3, 5, 7)}
    assert all(v > 0 for v in w.values()) and w[1] > w[0] and w[5] > w[1] and w[7] > w[3]
    pp = 2 * 12 * 1408 * 1408 * 4  # one [batch * heads, Tp, Tp] fp32 matrix
    assert w[1] - w[3] >= 2 * pp, (w, pp)
    # the step refuses a mode outside the set too (null pointers: nothing is launched either way)
    assert L.dvt_s2_train_step_mp(C.byref(c), None, None, None, None, None, 2, None, 0, None, None, 2) < 0


# ---- engine, Denoiser, command line ------------------------------------------------------------------------------------
def test_make_config_padding():
    from dvt_amd import s2
    assert [s2.make_config(768, t).tokens_pad for t in (1369, 121, 45, 64)] == [1408, 128, 64, 64]  # as ever
    assert [s2.make_config(768, t, row_pad=128).tokens_pad for t in (1369, 121, 45, 144)] == [1408, 128, 128, 256]
    with pytest.raises(ValueError):
        s2.make_config(768, 49, row_pad=32)


def test_engine_and_denoiser_refuse_by_name_before_a_device():
    """attention / weight_grad without the bf16 GEMM mode: refused with the texts stage 3 uses, before the device check (a CPU
    device would raise its own error first otherwise); unknown values likewise."""
    from dvt_amd import _lib, s2, s3
    from dvt_amd.models import Denoiser
    assert s2.ATTENTION_NEEDS_BF16 == s3.ATTENTION_NEEDS_BF16 and s2.WEIGHT_GRAD_NEEDS_BF16 == s3.WEIGHT_GRAD_NEEDS_BF16
    cfg = s2.make_config(384, 49)
    cpu = torch.device("cpu")
    with pytest.raises(_lib.DvtError, match="--attention bfloat16 needs --dtype bfloat16"):
        s2.Stage2Engine(cfg, cpu, attention="bfloat16")
    with pytest.raises(_lib.DvtError, match="--weight_grad bfloat16 needs --dtype bfloat16"):
        s2.Stage2Engine(cfg, cpu, weight_grad="bfloat16")
    with pytest.raises(_lib.DvtError, match="got dtype='float16'"):
        s2.Stage2Engine(cfg, cpu, dtype="float16")
    with pytest.raises(_lib.DvtError, match="needs a HIP device"):  # the defaults reach the device check
        s2.Stage2Engine(cfg, cpu)
    with pytest.raises(_lib.DvtError, match="--attention bfloat16 needs --dtype bfloat16"):
        Denoiser(7, 7, 384, None, device="cpu", train_attention="bfloat16")
    with pytest.raises(_lib.DvtError, match="--weight_grad bfloat16 needs --dtype bfloat16"):
        Denoiser(7, 7, 384, None, device="cpu", train_weight_grad="bfloat16")
    assert [s2.gemm_mode(), s2.gemm_mode("bfloat16"), s2.gemm_mode("bfloat16", "bfloat16"),
            s2.gemm_mode("bfloat16", weight_grad="bfloat16"), s2.gemm_mode("bfloat16", "bfloat16", "bfloat16")] == [0, 1, 3, 5, 7]


def test_engine_and_denoiser_defaults():
    import inspect
    from dvt_amd import s2
    from dvt_amd.models import Denoiser
    e = inspect.signature(s2.Stage2Engine.__init__).parameters
    assert [e[k].default for k in ("inference_only", "dtype", "attention", "weight_grad")] == [False, "float32", "float32", "float32"]
    d = inspect.signature(Denoiser.__init__).parameters
    assert [d[k].default for k in ("train_dtype", "train_attention", "train_weight_grad", "inference_dtype")] == ["float32"] * 4
    assert inspect.signature(s2.make_config).parameters["row_pad"].default == 64


def test_stage2_cli():
    from dvt_amd import stage2
    a = stage2.get_args([])
    assert (a.dtype, a.attention, a.weight_grad) == ("float32", "float32", "float32")
    a = stage2.get_args(["--dtype", "bfloat16", "--attention", "bfloat16", "--weight_grad", "bfloat16"])
    assert (a.dtype, a.attention, a.weight_grad) == ("bfloat16", "bfloat16", "bfloat16")
    with pytest.raises(SystemExit, match="stage 2: .*--attention bfloat16 needs --dtype bfloat16"):
        stage2.get_args(["--attention", "bfloat16"])
    with pytest.raises(SystemExit, match="stage 2: .*--weight_grad bfloat16 needs --dtype bfloat16"):
        stage2.get_args(["--weight_grad", "bfloat16"])
    with pytest.raises(SystemExit):
        stage2.get_args(["--dtype", "float16"])


# ---- stage 3: --teacher_dtype ------------------------------------------------------------------------------------------
S3_ARGS = ["--denoiser_ckpt", "unused.pth", "--model", "vit_small_patch14_dinov2.lvd142m", "--input_size", "56", "56"]


def test_teacher_dtype_argument():
    from dvt_amd import stage3
    assert stage3.get_args(S3_ARGS).teacher_dtype == "float32"
    assert stage3.get_args(S3_ARGS + ["--teacher_dtype", "bfloat16"]).teacher_dtype == "bfloat16"
    with pytest.raises(SystemExit):
        stage3.get_args(S3_ARGS + ["--teacher_dtype", "float16"])


@pytest.mark.parametrize("teacher_dtype", ["float32", "bfloat16"])
def test_build_models_hands_the_teacher_dtype_on(monkeypatch, tmp_path, teacher_dtype):
    """`build_models` with stand-in wrapper, Denoiser and engine classes: the wrapper gets dtype=teacher_dtype, the Denoiser
    inference_dtype="bfloat16" for the bf16 teacher and NO inference_dtype for the fp32 one (the call is today's), and the
    student is loaded from the wrapper's fp32 `_state_dict` either way."""
    from dvt_amd import s3, stage3
    from dvt_amd.models import online_denoiser, vit_wrapper
    from dvt_amd.vit import random_state_dict
    seen = {}
    sd = random_state_dict(384, 12, 14, 1 + 16, seed=0)

    class Wrapper:
        def __init__(self, model, **kw):
            seen["wrapper"] = kw
            self.dtype = kw["dtype"]
            self._state_dict = sd

    class FakeDenoiser:
        def __init__(self, *a, **kw):
            seen["denoiser"] = (a, kw)

        def load_state_dict(self, state, strict=True):
            seen["loaded"] = (set(state), strict)

    class Engine:
        def __init__(self, cfg, device, **kw):
            seen["engine"] = kw

        def load_timm(self, state):
            seen["student"] = state

    monkeypatch.setattr(vit_wrapper, "PretrainedViTWrapper", Wrapper)
    monkeypatch.setattr(online_denoiser, "Denoiser", FakeDenoiser)
    monkeypatch.setattr(s3, "Stage3Engine", Engine)
    ck = str(tmp_path / "den.pth")
    torch.save({"denoiser": {"pos_embed": torch.zeros(1, 16, 384), "denoiser.norm1.weight": torch.ones(384)}}, ck)
    args = stage3.get_args(S3_ARGS[2:] + ["--denoiser_ckpt", ck, "--teacher_dtype", teacher_dtype, "--allow_random_vit"])
    student, teacher = stage3.build_models(args, torch.device("cpu"))
    assert isinstance(student, Engine) and isinstance(teacher, FakeDenoiser)
    assert seen["wrapper"]["dtype"] == teacher_dtype
    a, kw = seen["denoiser"]
    assert a == (4, 4) and isinstance(kw["vit"], Wrapper) and kw["enable_pe"] is True
    if teacher_dtype == "bfloat16":
        assert kw["inference_dtype"] == "bfloat16"
    else:
        assert "inference_dtype" not in kw
    assert seen["loaded"][1] is False
    assert seen["student"] is sd and all(v.dtype == torch.float32 for v in sd.values())
    assert seen["engine"]["dtype"] == "float32"  # the student's modes do not follow the teacher's

    legacy = types.SimpleNamespace(**{k: v for k, v in vars(args).items() if k != "teacher_dtype"})
    stage3.build_models(legacy, torch.device("cpu"))  # a namespace from before the switch: the fp32 teacher
    assert seen["wrapper"]["dtype"] == "float32" and "inference_dtype" not in seen["denoiser"][1]
