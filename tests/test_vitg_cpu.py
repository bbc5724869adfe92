"""CPU: the ViT-g/14 backbone (SwiGLU MLP, dim 1536) -- reference restatement, wrapper, packing, ABI, refusals.

No GPU is touched: the float64 reference of tests/vitg_reference.py is held against transformers' Dinov2 models with
use_swiglu_ffn=True, the wrapper is built on random weights, the row permutation of the packed SwiGLU fc1 is inverted, and
the C ABI's host functions are called through ctypes.
"""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import pytest
import torch

from tests import vitg_reference as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIANTS = [("vit_giant_patch14_dinov2.lvd142m", 0), ("vit_giant_patch14_reg4_dinov2.lvd142m", 4)]


# ------------------------------------------------------------------------------------------ restatement vs transformers
@pytest.mark.parametrize("dim,depth,img,n_reg", [(128, 2, 56, 0), (192, 3, 70, 4)])
def test_vitg_reference_equals_hf_swiglu(dim, depth, img, n_reg):
    pytest.importorskip("transformers")
    from dvt_amd.vit import random_state_dict, swiglu_hidden
    g = img // 14
    sd = random_state_dict(dim, depth, 14, (0 if n_reg else 1) + g * g, seed=3, well_conditioned=True, n_reg=n_reg, mlp="swiglu")
    hid = swiglu_hidden(dim)
    assert sd["blocks.0.mlp.fc1.weight"].shape == (2 * hid, dim) and sd["blocks.0.mlp.fc2.weight"].shape == (dim, hid)
    x = torch.randn(2, 3, img, img, generator=torch.Generator().manual_seed(0))
    mine = vref.forward_features(sd, x, 14, 14, dtype=torch.float32)
    hf = vref.to_hf_dinov2_swiglu(sd, img, 14)
    assert hf.encoder.layer[0].mlp.weights_in.weight.shape == (2 * hid, dim)
    with torch.no_grad():
        ref = hf(pixel_values=x).last_hidden_state[:, 1 + n_reg:].reshape(2, g, g, dim)
    torch.testing.assert_close(mine, ref, rtol=1e-5, atol=1e-5)
    # ... and the float64 default is the same function (what is left is the fp32 evaluation's own rounding)
    torch.testing.assert_close(vref.forward_features(sd, x, 14, 14).float(), mine, rtol=1e-4, atol=1e-4)


def test_vitg_reference_layer_stride_cls_and_gelu_path():
    from dvt_amd.vit import random_state_dict
    from oracle import vit as ovit
    sd = random_state_dict(128, 3, 14, 1 + 16, seed=0, well_conditioned=True, mlp="swiglu")
    x = torch.randn(1, 3, 56, 56, generator=torch.Generator().manual_seed(2))
    a = vref.forward_features(sd, x, 14, 14, n_blocks=2)
    b, cls = vref.forward_features(sd, x, 14, 14, n_blocks=3, return_cls=True)
    assert a.shape == b.shape == (1, 4, 4, 128) and cls.shape == (1, 128) and not torch.allclose(a, b)
    assert vref.forward_features(sd, x, 14, 7).shape == (1, 7, 7, 128)
    # a GELU state dict through the same code equals the project's oracle
    sdg = random_state_dict(128, 2, 14, 1 + 16, seed=1, well_conditioned=True)
    torch.testing.assert_close(vref.forward_features(sdg, x, 14, 7, dtype=torch.float32), ovit.forward_features(sdg, x, 14, 7),
                               rtol=1e-5, atol=1e-5)


# ----------------------------------------------------------------------------------------------------------- the wrapper
@pytest.mark.parametrize("model,n_reg", GIANTS)
def test_wrapper_builds_the_giant_models_on_the_cpu(model, n_reg):
    from dvt_amd.models import PretrainedViTWrapper
    with pytest.warns(UserWarning, match="RANDOM ViT weights"):
        w = PretrainedViTWrapper(model, stride=14, allow_random_init=True)
    assert (w.n_output_dims, w.num_blocks, w.last_layer_index, w.patch_size) == (1536, 40, 39, 14)
    sd = w._state_dict
    assert sd["pos_embed"].shape == (1, (0 if n_reg else 1) + 37 * 37, 1536)
    assert ("reg_token" in sd) == bool(n_reg)
    if n_reg:
        assert sd["reg_token"].shape == (1, 4, 1536)
    for i in (0, 39):
        p = f"blocks.{i}."
        assert sd[p + "mlp.fc1.weight"].shape == (8192, 1536) and sd[p + "mlp.fc1.bias"].shape == (8192,)
        assert sd[p + "mlp.fc2.weight"].shape == (1536, 4096) and sd[p + "mlp.fc2.bias"].shape == (1536,)
        assert sd[p + "attn.qkv.weight"].shape == (4608, 1536) and sd[p + "ls2.gamma"].shape == (1536,)
    assert "blocks.40.norm1.weight" not in sd


def _sd_hash(sd):
    m = hashlib.sha256()
    for k in sorted(sd):
        m.update(k.encode())
        m.update(sd[k].contiguous().numpy().tobytes())
    return m.hexdigest()


def test_random_state_dict_default_is_bit_identical_to_the_parent():
    """sha256 over the sorted (key, bytes) pairs, computed on the commit before the `mlp` argument existed."""
    from dvt_amd.vit import random_state_dict
    assert _sd_hash(random_state_dict(128, 2, 14, 17, seed=1, well_conditioned=True)) == \
        "0730feb54d2a1db9f5efbeb5f1446f4ec19a2ee1e654ca786db132c767221658"
    assert _sd_hash(random_state_dict(192, 3, 14, 25, seed=3, well_conditioned=False, n_reg=4)) == \
        "7dcf57560cb3d992e23c15648670d4dc0c602a44ba05e874846fde1a83129d10"
    assert _sd_hash(random_state_dict(384, 1, 14, 1370, seed=0, well_conditioned=True)) == \
        "6670e618ffdd938f1e33b27b6b8f7cb022608bea010e6e32e35317f3ac3368c9"
    assert _sd_hash(random_state_dict(128, 2, 14, 17, seed=1, well_conditioned=True, mlp="gelu")) == \
        "0730feb54d2a1db9f5efbeb5f1446f4ec19a2ee1e654ca786db132c767221658"


# --------------------------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize("hid", [64, 512, 4096])
def test_swiglu_packing_roundtrip_and_layout(built_lib, hid):
    from dvt_amd.vit import swiglu_pack, swiglu_pack_index, swiglu_unpack
    idx = swiglu_pack_index(hid)
    assert sorted(idx.tolist()) == list(range(2 * hid))  # a permutation
    # the documented layout: of every 64 packed rows, 32 gates then the 32 values of the SAME hidden units
    blk = idx.reshape(-1, 64)
    assert torch.equal(blk[:, :32], torch.arange(hid).reshape(-1, 32))
    assert torch.equal(blk[:, 32:], blk[:, :32] + hid)
    # the C helper agrees entry by entry (and refuses what it cannot place)
    step = max(1, (2 * hid) // 257)
    for p in list(range(0, 2 * hid, step)) + [2 * hid - 1]:
        assert built_lib.dvt_vit_swiglu_pack_index(p, hid) == int(idx[p])
    assert built_lib.dvt_vit_swiglu_pack_index(2 * hid, hid) == -1
    assert built_lib.dvt_vit_swiglu_pack_index(0, hid + 8) == -1
    w = torch.randn(2 * hid, 24, generator=torch.Generator().manual_seed(hid))
    assert torch.equal(swiglu_unpack(swiglu_pack(w)), w)
    assert torch.equal(swiglu_pack(w)[64:96], w[32:64]) and torch.equal(swiglu_pack(w)[96:128], w[hid + 32:hid + 64])
    b = torch.randn(2 * hid)
    assert torch.equal(swiglu_unpack(swiglu_pack(b)), b)


def test_fold_commutes_with_the_packing():
    """Folded weights, column sums and folded bias are row-local: fold then pack == pack then fold, bit for bit."""
    from dvt_amd.vit import fold_layernorm, swiglu_pack
    g = torch.Generator().manual_seed(7)
    hid, dim = 256, 192
    W, b = torch.randn(2 * hid, dim, generator=g) * 0.1, torch.randn(2 * hid, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(dim, generator=g), 0.2 * torch.randn(dim, generator=g)
    Wf, cs, bf = fold_layernorm(W, b, gamma, beta)
    Wf2, cs2, bf2 = fold_layernorm(swiglu_pack(W), swiglu_pack(b), gamma, beta)
    assert torch.equal(swiglu_pack(Wf).view(torch.int16), Wf2.view(torch.int16))
    assert torch.equal(swiglu_pack(cs), cs2)
    torch.testing.assert_close(swiglu_pack(bf), bf2, rtol=0, atol=1e-6)  # (W @ beta: the matmul may block rows differently)


# ------------------------------------------------------------------------------------------------------------------- ABI
def _cfg_tuple(c):
    return tuple(getattr(c, n) for n, _ in type(c)._fields_)


def test_config_abi(built_lib):
    from dvt_amd.vit import MLP_SWIGLU, SPECS, VitBlockWeights, VitConfig, VitWeights, vit_config
    L = built_lib
    sizes = (C.c_int64 * 3)()
    assert L.dvt_vit_struct_sizes(sizes) == 0
    assert list(sizes) == [C.sizeof(VitConfig), C.sizeof(VitBlockWeights), C.sizeof(VitWeights)]
    assert C.sizeof(VitConfig) == 17 * 4
    # the six S / B / L specs: what dvt_vit_config_reg wrote before the field existed, and mlp_kind = 0 behind it
    for name, s in SPECS.items():
        if s.mlp != "gelu":
            continue
        a, b = VitConfig(), VitConfig()
        assert L.dvt_vit_config_reg(s.dim, s.depth, 14, 14, 518, 518, s.n_reg, C.byref(a)) == 0
        n_tok = 1 + s.n_reg + 37 * 37
        want = (s.dim, s.depth, s.dim // 64, 4 * s.dim, 14, 14, 518, 518, 37, 37, n_tok, (n_tok + 127) // 128 * 128, 640,
                1 + s.n_reg, a.ln_eps, int(s.n_reg == 0), 0)
        assert _cfg_tuple(a) == want and abs(a.ln_eps - 1e-6) < 1e-12, name
        assert L.dvt_vit_config_ex(s.dim, s.depth, 14, 14, 518, 518, s.n_reg, 0, C.byref(b)) == 0
        assert bytes(a) == bytes(b)
        if s.n_reg == 0:
            c = VitConfig()
            assert L.dvt_vit_config(s.dim, s.depth, 14, 14, 518, 518, C.byref(c)) == 0 and bytes(c) == bytes(a)
    # ViT-g
    for n_reg in (0, 4):
        g = VitConfig()
        assert L.dvt_vit_config_ex(1536, 40, 14, 14, 518, 518, n_reg, MLP_SWIGLU, C.byref(g)) == 0
        assert (g.dim, g.depth, g.heads, g.mlp_dim, g.mlp_kind, g.n_prefix, g.pos_has_cls) == \
            (1536, 40, 24, 4096, 1, 1 + n_reg, int(n_reg == 0))
        assert g.n_tokens == 1 + n_reg + 1369 and g.s_pad == 1408
        # workspace: hid is half of what a GELU MLP of the same fc1 width would need; every path sizes it
        assert L.dvt_vit_workspace_bytes(C.byref(g), 2) > 0 and L.dvt_vit_workspace_bytes_f32(C.byref(g), 2) > 0
        assert L.dvt_vit_workspace_bytes_f32x3(C.byref(g), 2) == -1  # bf16x3: refused
    assert L.dvt_vit_config_ex(1536, 40, 14, 14, 518, 518, 0, 2, C.byref(VitConfig())) == -1  # unknown MLP kind
    assert L.dvt_vit_config_ex(1664, 40, 14, 14, 518, 518, 0, 1, C.byref(VitConfig())) == -1  # wider than the row kernels
    assert vit_config(1536, 40, 14, 14, 518, 518, mlp="swiglu").mlp_dim == 4096
    # the forwards refuse a bf16x3 SwiGLU config by return code, before touching any pointer
    g = vit_config(1536, 40, 14, 14, 518, 518, mlp="swiglu")
    w = VitWeights()
    assert L.dvt_vit_forward_f32x3(C.byref(g), C.byref(w), 256, 256, 1, 1, 256, None) == -1


# -------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("model,_n", GIANTS)
def test_stage1_cli_refuses_the_giant_models_before_writing(tmp_path, model, _n):
    save, out = tmp_path / "save", tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "denoising-vit_amd"), ROOT]))
    r = subprocess.run([sys.executable, "-m", "dvt_amd.stage1", "--model", model, "--save_root", str(save), "--output_dir",
                        str(out), "--data_root", str(tmp_path / "data"), "--synthetic", "--num_imgs", "1"],
                       capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert r.returncode != 0
    assert model in r.stderr and "feat_dim 1536" in r.stderr, r.stderr[-2000:]
    assert sorted(p.name for p in tmp_path.iterdir()) == [], "the refusal must come before anything is written"


def test_matmul_high_with_swiglu_is_refused_by_name():
    """HipViT names the model family and matmul="high"; the refusal precedes every device call."""
    from dvt_amd._lib import DvtError
    from dvt_amd.vit import HipViT, random_state_dict
    sd = random_state_dict(1536, 1, 14, 1 + 16, seed=0, mlp="swiglu")
    with pytest.raises(DvtError, match=r"vit_giant_patch14.*matmul=\"high\""):
        HipViT(sd, 14, 14, (56, 56), "cpu", dtype="float32", matmul="high")
    with pytest.raises(DvtError, match="needs a HIP device"):  # (the other modes get as far as the device check)
        HipViT(sd, 14, 14, (56, 56), "cpu", dtype="float32")


@pytest.mark.parametrize("model,_n", GIANTS)
def test_every_consumer_refuses_the_giant_models_with_the_limit_named(tmp_path, monkeypatch, model, _n):
    """evaluate, visualize, video_demo and stage2 stop on a giant id with the model, "feat_dim 1536" and the limit (1024) in
    the message, before a device is touched or a file is written."""
    import argparse

    from dvt_amd import evaluate, stage2, video_demo, visualize
    from dvt_amd._lib import DvtError
    pat = rf"{model}.*feat_dim 1536.*feat_dim <= 1024"
    monkeypatch.chdir(tmp_path)
    for task, cfg in (("segmentation", "voc2012_linear"), ("depth", "nyu_linear")):
        with pytest.raises(DvtError, match=pat):
            evaluate.main([cfg, "--task", task, "--backbone-type", model, "--allow_random_vit", "--launcher", "none",
                           "--work-dir", str(tmp_path / "work")])
    with pytest.raises(DvtError, match=pat):
        visualize.main(argparse.Namespace(model=model, save_root=str(tmp_path / "save"), output_dir=str(tmp_path / "vis"),
                                          data_root=None, img_path=None, start_idx=0, num_imgs=1, panel_size=518,
                                          num_clusters=5, seed=0), device=torch.device("cpu"))
    with pytest.raises(DvtError, match=pat):
        video_demo.plan(argparse.Namespace(model=model, vit_checkpoint=None, allow_random_vit=True, fps=10, height=490,
                                           width=854, stride_size=4, stats=str(tmp_path / "stats.pth"), stats_prefix="",
                                           num_clusters=8, frames=[str(tmp_path / "scene")]))
    with pytest.raises(DvtError, match=pat):
        stage2.model_geometry(argparse.Namespace(model=model, input_size=(518, 518), stride_size=14))
    assert sorted(q.name for q in tmp_path.iterdir()) == [], "a refusal must come before anything is written"

