"""CPU: the DINO / DeiT-III / AugReg patch-8 / patch-16 backbones -- spec table, reference restatement, wrapper, statistics,
refusals.  No GPU is touched: the float64 reference of tests/backbone_reference.py is held against the project's oracle and
against transformers.ViTModel, the wrapper is built on random weights, and the consumers' host functions are called directly.
"""
import argparse
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from tests import backbone_reference as bref

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
# id: (dim, depth, patch, img, LayerScale keys, position table has a cls row, (mean, std))
TABLE = {
    "vit_small_patch16_224.dino": (384, 12, 16, 224, False, 1, IMAGENET),
    "vit_small_patch8_224.dino": (384, 12, 8, 224, False, 1, IMAGENET),
    "vit_base_patch16_224.dino": (768, 12, 16, 224, False, 1, IMAGENET),
    "vit_base_patch8_224.dino": (768, 12, 8, 224, False, 1, IMAGENET),
    "deit3_base_patch16_224.fb_in1k": (768, 12, 16, 224, True, 0, IMAGENET),
    "vit_base_patch16_384.augreg_in21k_ft_in1k": (768, 12, 16, 384, False, 1, HALF),
}
# the eight entries of the parent commit: (dim, depth, patch, img_size, ls_init, n_reg, mlp)
PARENT = {
    "vit_small_patch14_dinov2.lvd142m": (384, 12, 14, 518, 1e-5, 0, "gelu"),
    "vit_base_patch14_dinov2.lvd142m": (768, 12, 14, 518, 1e-5, 0, "gelu"),
    "vit_large_patch14_dinov2.lvd142m": (1024, 24, 14, 518, 1e-5, 0, "gelu"),
    "vit_small_patch14_reg4_dinov2.lvd142m": (384, 12, 14, 518, 1e-5, 4, "gelu"),
    "vit_base_patch14_reg4_dinov2.lvd142m": (768, 12, 14, 518, 1e-5, 4, "gelu"),
    "vit_large_patch14_reg4_dinov2.lvd142m": (1024, 24, 14, 518, 1e-5, 4, "gelu"),
    "vit_giant_patch14_dinov2.lvd142m": (1536, 40, 14, 518, 1e-5, 0, "swiglu"),
    "vit_giant_patch14_reg4_dinov2.lvd142m": (1536, 40, 14, 518, 1e-5, 4, "swiglu"),
}
REFUSED = ["vit_base_patch16_224.mae", "vit_base_patch16_clip_384.laion2b_ft_in12k_in1k", "vit_base_patch16_clip_224.openai",
           "eva02_base_patch16_clip_224.merged2b"]


# ------------------------------------------------------------------------------------------------------------ the table
def test_spec_table():
    from dvt_amd.vit import SPECS, VitSpec
    assert set(SPECS) == set(TABLE) | set(PARENT)
    for name, (dim, depth, patch, img, ls, cls_row, (mean, std)) in TABLE.items():
        s = SPECS[name]
        assert (s.dim, s.depth, s.patch, s.img_size, s.layer_scale, s.pos_has_cls, s.n_reg, s.mlp) == \
            (dim, depth, patch, img, ls, cls_row, 0, "gelu"), name
        assert (tuple(s.mean), tuple(s.std)) == (mean, std), name
        assert s.n_pos == cls_row + (img // patch) ** 2
    for name, (dim, depth, patch, img, ls_init, n_reg, mlp) in PARENT.items():
        s = SPECS[name]
        assert (s.dim, s.depth, s.patch, s.img_size, s.ls_init, s.n_reg, s.mlp) == (dim, depth, patch, img, ls_init, n_reg, mlp)
        # what the parent derived or hard-coded for them is what the new fields default to
        assert (s.pos_has_cls, s.layer_scale, (tuple(s.mean), tuple(s.std))) == (int(n_reg == 0), True, IMAGENET), name
        assert s == VitSpec(dim, depth, n_reg=n_reg, mlp=mlp), name
    assert SPECS["deit3_base_patch16_224.fb_in1k"].n_reg == 0  # no cls row AND no registers: not derivable from n_reg


def test_random_state_dict_layouts():
    from dvt_amd.vit import random_state_dict
    full = random_state_dict(128, 2, 16, 1 + 4, seed=2, well_conditioned=True)
    bare = random_state_dict(128, 2, 16, 1 + 4, seed=2, well_conditioned=True, layer_scale=False)
    assert not any(".ls" in k for k in bare) and set(full) - set(bare) == {f"blocks.{i}.{n}.gamma" for i in (0, 1)
                                                                          for n in ("ls1", "ls2")}
    assert bare["pos_embed"].shape == (1, 5, 128) and bare["patch_embed.proj.weight"].shape == (128, 3, 16, 16)
    assert random_state_dict(128, 1, 8, 9, seed=2, layer_scale=False)["pos_embed"].shape == (1, 9, 128)  # no cls row


# ------------------------------------------------------------------------------------------- restatement vs the oracle
@pytest.mark.parametrize("dim,patch,img,stride", [(128, 16, 64, 16), (128, 8, 48, 8), (192, 16, 64, 8), (128, 8, 40, 4)])
def test_reference_equals_the_oracle_on_the_dino_layout(dim, patch, img, stride):
    """cls + patches table, no LayerScale: the fp32 evaluation of the restatement against oracle/vit.py (fp32), to float32
    round-off; the float64 default is the same function."""
    from dvt_amd.vit import random_state_dict
    from oracle import vit as ovit
    g0 = img // patch
    sd = random_state_dict(dim, 2, patch, 1 + g0 * g0, seed=dim + stride, well_conditioned=True, layer_scale=False)
    x = torch.randn(2, 3, img, img, generator=torch.Generator().manual_seed(1))
    want = ovit.forward_features(sd, x, patch, stride)
    g = (img - patch) // stride + 1
    mine = bref.forward_features(sd, x, patch, stride, dtype=torch.float32)
    assert mine.shape == want.shape == (2, g, g, dim)
    torch.testing.assert_close(mine, want, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(bref.forward_features(sd, x, patch, stride).float(), mine, rtol=1e-4, atol=1e-4)
    a, cls = bref.forward_features(sd, x, patch, stride, n_blocks=1, return_cls=True)
    assert cls.shape == (2, dim) and not torch.allclose(a.float(), mine)


@pytest.mark.parametrize("dim,patch,img", [(128, 16, 64), (192, 8, 48)])
def test_reference_equals_hf_vit(dim, patch, img):
    try:
        from transformers import ViTModel  # noqa: F401
    except Exception as exc:  # noqa: BLE001
        pytest.skip(f"transformers.ViTModel cannot be imported: {exc!r}")
    from dvt_amd.vit import random_state_dict
    g = img // patch
    sd = random_state_dict(dim, 3, patch, 1 + g * g, seed=5, well_conditioned=True, layer_scale=False)
    x = torch.randn(2, 3, img, img, generator=torch.Generator().manual_seed(0))
    hf = bref.to_hf_vit(sd, img, patch)
    with torch.no_grad():
        out = hf(pixel_values=x).last_hidden_state
    mine, cls = bref.forward_features(sd, x, patch, patch, dtype=torch.float32, return_cls=True)
    torch.testing.assert_close(mine, out[:, 1:].reshape(2, g, g, dim), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(cls, out[:, 0], rtol=1e-5, atol=1e-5)


def test_deit3_layout_by_construction():
    """No cls row in the table (and no registers): pos_embed reaches the patch rows of block 0's input only, cls_token row 0
    only, and the cls row is the cls token itself."""
    from dvt_amd.vit import random_state_dict
    sd = random_state_dict(128, 1, 16, 9, seed=3, well_conditioned=True)  # 3 x 3 grid, LayerScale keys present
    assert bref.pos_has_cls(sd) == 0 and "blocks.0.ls1.gamma" in sd
    x = torch.randn(2, 3, 48, 48, generator=torch.Generator().manual_seed(4))
    base, gh, gw = bref.embed(sd, x, 16)
    assert base.shape == (2, 10, 128) and (gh, gw) == (3, 3)
    assert torch.equal(base[:, 0], sd["cls_token"].double().reshape(1, 128).expand(2, -1))
    sd2 = dict(sd, pos_embed=sd["pos_embed"] + 1.0)
    moved = bref.embed(sd2, x, 16)[0]
    assert torch.equal(moved[:, 0], base[:, 0]) and torch.allclose(moved[:, 1:], base[:, 1:] + 1.0, rtol=0, atol=1e-6)
    sd3 = dict(sd, cls_token=sd["cls_token"] + 1.0)
    moved = bref.embed(sd3, x, 16)[0]
    assert torch.equal(moved[:, 1:], base[:, 1:]) and torch.allclose(moved[:, 0], base[:, 0] + 1.0, rtol=0, atol=1e-6)
    # with a stride override the table is resampled with no prefix row: 5 x 5 grid from the 3 x 3 table
    over, gh, gw = bref.embed(sd, x, 8)
    assert (gh, gw) == (5, 5) and over.shape == (2, 26, 128) and torch.equal(over[:, 0], base[:, 0])
    # LayerScale is applied: doubling ls2 changes the output
    a = bref.forward_features(sd, x, 16, 16)
    b = bref.forward_features(dict(sd, **{"blocks.0.ls2.gamma": sd["blocks.0.ls2.gamma"] * 2}), x, 16, 16)
    assert a.shape == (2, 3, 3, 128) and not torch.allclose(a, b)


# ----------------------------------------------------------------------------------------------------------- the wrapper
@pytest.mark.parametrize("model", sorted(TABLE))
def test_wrapper_builds_the_six_models_on_the_cpu(model):
    """FAILS on the parent commit: NotImplementedError for every one of the six ids."""
    from dvt_amd.models import PretrainedViTWrapper
    dim, depth, patch, img, ls, cls_row, (mean, std) = TABLE[model]
    with pytest.warns(UserWarning, match="RANDOM ViT weights"):
        w = PretrainedViTWrapper(model, stride=patch, allow_random_init=True)
    assert (w.n_output_dims, w.num_blocks, w.last_layer_index, w.patch_size) == (dim, depth, depth - 1, patch)
    assert w.img_size == (img, img)
    assert tuple(w.model.pos_embed.shape) == (1, cls_row + (img // patch) ** 2, dim)
    norm = w.transformation.transforms[-1]
    assert (tuple(norm.mean), tuple(norm.std)) == (mean, std)
    sd = w._state_dict
    assert ("blocks.0.ls1.gamma" in sd) == ls and ("blocks.%d.ls2.gamma" % (depth - 1) in sd) == ls
    assert "reg_token" not in sd and sd["patch_embed.proj.weight"].shape == (dim, 3, patch, patch)
    assert sd["blocks.0.mlp.fc1.weight"].shape == (4 * dim, dim)
    # the transformation normalises with the model's own numbers
    px = torch.full((3, 2, 2), 0.5)
    torch.testing.assert_close(w.transformation(px), (px - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1))


@pytest.mark.parametrize("model", REFUSED)
def test_the_other_families_are_still_refused(model):
    from dvt_amd.models import PretrainedViTWrapper
    with pytest.raises(NotImplementedError, match=model.split(".")[0]):
        PretrainedViTWrapper(model, stride=16, allow_random_init=True)


def test_the_refusal_names_why():
    from dvt_amd.models import PretrainedViTWrapper
    for model, word in (("vit_base_patch16_clip_224.openai", "norm_pre"), ("eva02_base_patch16_clip_224.merged2b", "rotary"),
                        ("vit_base_patch16_224.mae", "MAE")):
        with pytest.raises(NotImplementedError, match=word):
            PretrainedViTWrapper(model, stride=16)


# ---------------------------------------------------------------------------------------------------- config and engine
def test_config_carries_pos_has_cls(built_lib):
    from dvt_amd._lib import DvtError
    from dvt_amd.vit import HipViT, VitConfig, random_state_dict, vit_config
    assert C.sizeof(VitConfig) == 17 * 4
    for patch, img, stride, k_patch, grid in ((16, 224, 16, 768, 14), (8, 224, 8, 192, 28), (16, 384, 16, 768, 24),
                                              (16, 224, 8, 768, 27)):
        c = vit_config(768, 12, patch, stride, img, img, row_pad=32)
        assert (c.patch, c.k_patch, c.grid_h, c.grid_w, c.n_tokens, c.n_prefix, c.pos_has_cls) == \
            (patch, k_patch, grid, grid, 1 + grid * grid, 1, 1)
        assert c.s_pad == -(-c.n_tokens // 32) * 32 and abs(c.ln_eps - 1e-6) < 1e-12
        d = vit_config(768, 12, patch, stride, img, img, row_pad=32, pos_has_cls=0)  # DeiT-III: no registers, no cls row
        assert (d.n_prefix, d.pos_has_cls) == (1, 0)
        d.pos_has_cls = 1
        assert bytes(d) == bytes(c)
        assert built_lib.dvt_vit_workspace_bytes(C.byref(c), 2) > 0 and built_lib.dvt_vit_workspace_bytes_f32(C.byref(c), 2) > 0
    assert vit_config(768, 12, 16, 16, 224, 224).s_pad == 256  # (the C side's own padding: 197 tokens -> 256 rows)
    with pytest.raises(DvtError, match="pos_has_cls"):
        vit_config(768, 12, 16, 16, 224, 224, pos_has_cls=2)
    # the engine reads the layout from the table's row count, before it asks for a device
    sd = random_state_dict(128, 1, 16, 4, seed=0)
    with pytest.raises(DvtError, match="needs a HIP device"):
        HipViT(sd, 16, 16, (32, 32), "cpu")
    with pytest.raises(DvtError, match="no cls row"):
        HipViT(random_state_dict(128, 1, 16, 4, seed=0, n_reg=4), 16, 16, (32, 32), "cpu", pos_has_cls=1)


# ----------------------------------------------------------------------------------------------------------- statistics
def _png_2x2(path):
    from PIL import Image
    a = np.array([[[0, 64, 128], [255, 255, 255]], [[10, 20, 30], [200, 100, 50]]], np.uint8)
    Image.fromarray(a).save(path)
    return a.astype(np.float32) / 255.0


def test_stage3_and_video_normalise_with_the_models_statistics(tmp_path):
    from dvt_amd import stage3, video_demo
    a = _png_2x2(str(tmp_path / "p.png"))
    aug, dino = "vit_base_patch16_384.augreg_in21k_ft_in1k", "vit_base_patch16_224.dino"
    assert stage3.model_statistics(aug) == HALF and video_demo.model_statistics(aug) == HALF
    assert stage3.model_statistics(dino) == IMAGENET and video_demo.model_statistics(dino) == IMAGENET
    assert stage3.model_statistics("vit_base_patch14_dinov2.lvd142m") == IMAGENET
    for stats in (HALF, IMAGENET):
        want = ((a - np.asarray(stats[0], np.float32)) / np.asarray(stats[1], np.float32)).transpose(2, 0, 1)
        got3 = stage3.load_image(str(tmp_path / "p.png"), (2, 2), False, *stats)
        gotv = video_demo.load_frame(str(tmp_path / "p.png"), 2, 2, *stats).numpy()
        np.testing.assert_allclose(got3, want, rtol=0, atol=1e-6)
        np.testing.assert_allclose(gotv, want, rtol=0, atol=1e-6)
    half = stage3.load_image(str(tmp_path / "p.png"), (2, 2), False, *stage3.model_statistics(aug))
    assert half.min() == -1.0 and half.max() == 1.0  # 0 -> -1, 255 -> 1: AugReg's range
    # the defaults are what they were
    np.testing.assert_array_equal(stage3.load_image(str(tmp_path / "p.png"), (2, 2), False),
                                  stage3.load_image(str(tmp_path / "p.png"), (2, 2), False, *IMAGENET))


# ------------------------------------------------------------------------------------------------------------- consumers
@pytest.mark.parametrize("model", sorted(TABLE))
def test_consumers_accept_or_refuse_by_name(tmp_path, monkeypatch, model):
    """stage 2 and the video demo take the six ids with the model's own geometry; the stage-3 trainer and the linear-probe
    evaluation refuse them by name before anything is written."""
    from dvt_amd import evaluate, stage2, stage3, video_demo
    from dvt_amd import video as VD
    from dvt_amd._lib import DvtError
    dim, depth, patch, img, ls, cls_row, _ = TABLE[model]
    monkeypatch.chdir(tmp_path)
    g = img // patch
    assert stage2.model_geometry(argparse.Namespace(model=model, input_size=(img, img), stride_size=patch)) == (dim, g, g)
    g2 = (img - patch) // (patch // 2) + 1
    assert stage2.model_geometry(argparse.Namespace(model=model, input_size=(img, img), stride_size=patch // 2)) == (dim, g2, g2)
    # video_demo.plan gets as far as the statistics file: model, weights and geometry were accepted
    monkeypatch.setattr(VD, "load_stats", lambda *a: (_ for _ in ()).throw(DvtError("stats reached")))
    with pytest.raises(DvtError, match="stats reached"):
        video_demo.plan(argparse.Namespace(model=model, vit_checkpoint=None, allow_random_vit=True, fps=10, height=img,
                                           width=img, stride_size=patch, stats=str(tmp_path / "stats.pth"), stats_prefix="",
                                           num_clusters=8, frames=[str(tmp_path / "scene")]))
    pat = rf"{model.split('.')[0]}.*DINOv2 patch-14.*nothing was written"
    with pytest.raises(DvtError, match=pat):
        stage3.geometry(argparse.Namespace(model=model, input_size=(img, img), stride_size=patch))
    for task, cfg in (("segmentation", "voc2012_linear"), ("depth", "nyu_linear")):
        with pytest.raises(DvtError, match=pat):
            evaluate.main([cfg, "--task", task, "--backbone-type", model, "--allow_random_vit", "--launcher", "none",
                           "--work-dir", str(tmp_path / "work")])
    assert sorted(q.name for q in tmp_path.iterdir()) == [], "a refusal must come before anything is written"


@pytest.mark.parametrize("model,patch", [("vit_small_patch8_224.dino", 8), ("vit_base_patch16_224.dino", 16),
                                         ("vit_base_patch14_dinov2.lvd142m", 14)])
def test_auto_stride_reads_any_patch_size(model, patch):
    """`--auto_stride` of the stage-2 and stage-3 drivers: the stride is the model's patch size, patch 8 included."""
    from dvt_amd import stage2, stage3
    size = str(16 * patch)
    a2 = stage2.get_args(["--model", model, "--auto_stride", "--input_size", size, size])
    a3 = stage3.get_args(["--model", model, "--auto_stride", "--input_size", size, size, "--denoiser_ckpt", "none.pth"])
    assert a2.stride_size == patch and a3.stride_size == patch


@pytest.mark.parametrize("has_cls", [0, 1])
@pytest.mark.parametrize("g0,new", [(3, (5, 5)), (14, (27, 27)), (7, (13, 13)), (4, (4, 4))])
def test_product_resample_equals_the_reference(g0, new, has_cls):
    """dvt_amd.vit.resample_pos_embed (what HipViT calls) against the reference's resample, bit for bit, with and without a
    cls row: with none (DeiT-III, no registers) the whole table is the grid, with one the first row is carried over."""
    from dvt_amd.vit import resample_pos_embed
    table = torch.randn(1, has_cls + g0 * g0, 64, generator=torch.Generator().manual_seed(g0))
    mine = resample_pos_embed(table, new, has_cls)
    want = bref.resample_pos(table, new, has_cls)
    assert mine.shape == (1, has_cls + new[0] * new[1], 64) and torch.equal(mine, want)
    if has_cls:
        assert torch.equal(mine[:, 0], table[:, 0])
    if (g0, g0) == new:
        assert torch.equal(mine, table)


def test_statistics_helper_is_one_function():
    from dvt_amd import stage3, video_demo, vit
    assert stage3.model_statistics is vit.model_statistics and video_demo.model_statistics is vit.model_statistics
    assert vit.model_statistics("not-a-model") == IMAGENET


def test_wrapper_default_models_are_unchanged():
    """The DINOv2 wrapper: ImageNet statistics, a 1370-row table, LayerScale keys -- as on the parent commit."""
    from dvt_amd.models import PretrainedViTWrapper
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = PretrainedViTWrapper("vit_small_patch14_dinov2.lvd142m", stride=14, allow_random_init=True)
    norm = w.transformation.transforms[-1]
    assert (tuple(norm.mean), tuple(norm.std)) == IMAGENET and tuple(w.model.pos_embed.shape) == (1, 1370, 384)
    assert "blocks.11.ls2.gamma" in w._state_dict
