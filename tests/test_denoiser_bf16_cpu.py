"""CPU: the float64 reference of the Denoiser's forward (tests/denoiser_reference.py) against a block built from torch.nn
primitives, and the plumbing of the opt-in bf16 inference path: the `Denoiser` keyword and its default, the evaluation CLI's
flag and its refusal, the new entry points in the library and in a header, the host-side configuration and its refusals."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch
import torch.nn as nn

from tests import denoiser_reference as dref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dvt_denoiser_config", "dvt_denoiser_struct_sizes", "dvt_denoiser_workspace_bytes", "dvt_denoiser_forward_bf16",
               "dvt_vit_workspace_bytes_denoised", "dvt_vit_forward_denoised"]


class _NNBlock(nn.Module):
    """A pre-norm transformer block from torch.nn primitives alone (nn.MultiheadAttention splits in_proj into q | k | v and
    heads as timm's Attention splits qkv)."""

    def __init__(self, dim):
        super().__init__()
        self.norm1, self.norm2 = nn.LayerNorm(dim, eps=1e-6), nn.LayerNorm(dim, eps=1e-6)
        self.attn = nn.MultiheadAttention(dim, dim // 64, bias=True, batch_first=True)
        self.fc1, self.act, self.fc2 = nn.Linear(dim, 4 * dim), nn.GELU(), nn.Linear(4 * dim, dim)

    def load(self, sd, p):
        with torch.no_grad():
            for mod, name in ((self.norm1, "norm1"), (self.norm2, "norm2"), (self.fc1, "mlp.fc1"), (self.fc2, "mlp.fc2"),
                              (self.attn.out_proj, "attn.proj")):
                mod.weight.copy_(sd[p + name + ".weight"])
                mod.bias.copy_(sd[p + name + ".bias"])
            self.attn.in_proj_weight.copy_(sd[p + "attn.qkv.weight"])
            self.attn.in_proj_bias.copy_(sd[p + "attn.qkv.bias"])

    def forward(self, x):
        h = self.norm1(x)
        x = x + self.attn(h, h, h, need_weights=False)[0]
        return x + self.fc2(self.act(self.fc1(self.norm2(x))))


@pytest.mark.parametrize("dim,grid,num_blocks,enable_pe", [(128, (3, 5), 1, True), (192, (4, 4), 2, True), (128, (2, 3), 1, False)])
def test_reference_equals_a_torch_nn_block(dim, grid, num_blocks, enable_pe):
    sd = dref.random_denoiser_state(dim, num_blocks, grid, seed=dim + num_blocks, enable_pe=enable_pe)
    assert ("pos_embed" in sd) == enable_pe and len(sd) == 12 * num_blocks + int(enable_pe)
    assert (("denoiser.norm1.weight" in sd) if num_blocks == 1 else ("denoiser.1.mlp.fc2.bias" in sd))
    feats = dref.layernorm_like_features(2, grid, dim, seed=3)
    x = feats.double().reshape(2, -1, dim)
    if enable_pe:
        x = x + sd["pos_embed"].double()
    for i in range(num_blocks):
        blk = _NNBlock(dim).double()
        blk.load(sd, dref.block_prefix(i, num_blocks))
        with torch.no_grad():
            x = blk(x)
    got = dref.forward(sd, feats, num_blocks)
    err = float((got - x.reshape(got.shape)).abs().max() / x.abs().max())
    print(f"reference vs torch.nn block (dim {dim}, {num_blocks} blocks): max error / max {err:.2e}")
    assert err < 1e-12
    # the comparator rounds matrix operands only: close to the reference, not equal to it
    cmp16 = dref.forward(sd, feats, num_blocks, round_bf16=True)
    rel = float((cmp16 - got).norm() / got.norm())
    assert 1e-5 < rel < 2e-2, rel


def test_reference_resamples_the_position_table():
    from dvt_amd.vit import resample_pos_embed
    sd = dref.random_denoiser_state(128, 1, (8, 8), seed=1)
    feats = dref.layernorm_like_features(1, (5, 13), 128, seed=2)
    moved = dict(sd, pos_embed=resample_pos_embed(sd["pos_embed"], (5, 13), 0))
    assert moved["pos_embed"].shape == (1, 65, 128)
    assert torch.equal(dref.forward(sd, feats, noise_map=(8, 8)), dref.forward(moved, feats))


def test_denoiser_keyword_default_is_float32():
    from dvt_amd.models.online_denoiser import Denoiser
    p = inspect.signature(Denoiser.__init__).parameters["inference_dtype"]
    assert p.default == "float32"
    with pytest.raises(ValueError, match="inference_dtype"):
        Denoiser(8, 8, 768, device="cuda", inference_dtype="float16")  # refused before a device is touched


def test_evaluate_flag_default_choices_and_refusal(capsys):
    from dvt_amd import evaluate
    a = evaluate.get_args(["voc2012_linear"])
    assert a.denoiser_dtype == "float32" and a.dtype == "bfloat16"
    assert evaluate.get_args(["voc2012_linear", "--denoiser_dtype", "bfloat16"]).denoiser_dtype == "bfloat16"
    assert evaluate.get_args(["voc2012_linear", "--dtype", "float32"]).denoiser_dtype == "float32"
    with pytest.raises(SystemExit):
        evaluate.get_args(["voc2012_linear", "--denoiser_dtype", "float16"])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        evaluate.get_args(["voc2012_linear", "--denoiser_dtype", "bfloat16", "--dtype", "float32"])
    err = capsys.readouterr().err
    assert "--denoiser_dtype bfloat16" in err and "--dtype float32" in err


def test_new_symbols_are_exported_and_declared(built_lib):
    header = open(os.path.join(ROOT, "include", "dvt_denoiser.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NEW_SYMBOLS:
        assert hasattr(built_lib, n), f"libdvt_hip.so lacks {n}"
        assert re.search(r"^\s*(?:int|int64_t)\s+" + n + r"\s*\(", header, flags=re.M), f"{n} is not declared in dvt_denoiser.h"


def test_host_config_and_refusals(built_lib):
    """dvt_denoiser_config and the workspace arithmetic are host functions: geometry, struct mirrors, and every refusal that
    needs no device pointer."""
    from dvt_amd import denoiser_bf16 as db
    from dvt_amd.vit import vit_config
    L = built_lib
    c = db.denoiser_config(768, 1, (37, 37), True, pad=32)
    assert (c.dim, c.heads, c.mlp_dim, c.n_blocks, c.n_tokens, c.s_pad, c.enable_pe) == (768, 12, 3072, 1, 1369, 1376, 1)
    assert db.denoiser_config(768, 2, (5, 13), True, pad=128).s_pad == 128 and db.denoiser_config(384, 1, (8, 8), False, pad=32).s_pad == 64
    assert L.dvt_denoiser_workspace_bytes(C.byref(c), 2) > 2 * 1376 * 768 * 4
    for args in ((512, 1, 5, 5, 1, 32), (1536, 1, 5, 5, 1, 32), (768, 0, 5, 5, 1, 32), (768, 9, 5, 5, 1, 32), (768, 1, 0, 5, 1, 32),
                 (768, 1, 5, 5, 1, 48), (768, 1, 5, 5, 1, 0)):
        assert L.dvt_denoiser_config(*args, C.byref(db.DenoiserConfig())) == -1, args
    assert L.dvt_denoiser_config(768, 1, 5, 5, 1, 32, None) == -1

    def bad(**kw):
        b = db.denoiser_config(768, 1, (5, 5), True, pad=32)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    for kw in (dict(s_pad=48), dict(s_pad=0), dict(n_tokens=24), dict(grid_w=6), dict(dim=512, heads=8, mlp_dim=2048),
               dict(heads=11), dict(mlp_dim=2048), dict(n_blocks=9)):
        assert L.dvt_denoiser_workspace_bytes(C.byref(bad(**kw)), 1) == -1, kw
    assert L.dvt_denoiser_workspace_bytes(C.byref(bad()), 0) == -1 and L.dvt_denoiser_workspace_bytes(None, 1) == -1
    # the fused workspace: the extractor's own bytes (unchanged) plus the denoiser's residual stream
    vc = vit_config(768, 2, 16, 16, 64, 64, row_pad=32)
    dc = db.denoiser_config(768, 1, (4, 4), True, pad=32)
    assert (vc.s_pad, dc.s_pad) == (32, 32)
    for batch in (1, 3):
        T2 = -(-batch * dc.s_pad // 256) * 256
        assert L.dvt_vit_workspace_bytes_denoised(C.byref(vc), C.byref(dc), batch) == \
            L.dvt_vit_workspace_bytes(C.byref(vc), batch) + T2 * 768 * 4
    assert L.dvt_vit_workspace_bytes_denoised(C.byref(vc), C.byref(db.denoiser_config(768, 1, (5, 5), True, pad=32)), 1) == -1
    assert L.dvt_vit_workspace_bytes_denoised(C.byref(vc), C.byref(db.denoiser_config(384, 1, (4, 4), True, pad=32)), 1) == -1
    assert L.dvt_vit_workspace_bytes_denoised(C.byref(vc), C.byref(db.denoiser_config(768, 1, (4, 4), True, pad=64)), 1) == -1
