"""GPU: the DINO / DeiT-III / AugReg patch-8 / patch-16 backbones on the HIP extractor -- im2col at patch 8 and 16 bit for
bit, the forward (bf16 and exact fp32) against the float64 reference of tests/backbone_reference.py at the token counts and
layouts these models bring, one full-depth ViT-B/16, and stage 1 end to end on ViT-S/16.

Bars (none of them comes from what the code under test gives): the small-depth forwards carry the bars of
tests/test_gpu_vit.py for the same dtype (bf16: per-token cosine > 0.999 and rel-L2 < 2e-2; fp32: rel-L2 < 2e-5 and cosine >
0.999999), the full-depth run its full-depth ViT-B bar (bf16: cosine min > 0.999).  Where a bf16 case misses them, `hold`
computes a CPU forward of the same arithmetic class (every matrix operand rounded to bf16) against the same float64
reference and allows twice ITS error, as tests/test_gpu_vitg.py does.
"""
import ctypes as C
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import backbone_reference as bref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN16, SENT16 = 0x7FC0, 0x5A5A


def _s():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def L(built_lib):
    import dvt_amd.vit  # noqa: F401 registers signatures
    return built_lib


# ------------------------------------------------------------------------------------------------------------- 1. im2col
@pytest.mark.parametrize("patch,stride", [(8, 8), (8, 4), (16, 16), (16, 8)])
def test_im2col_equals_unfold(L, patch, stride):
    """dvt_vit_im2col / dvt_vit_im2col_f32 (what the two forwards launch) on a 48 x 48 image, batch 2: every patch row equals
    torch's unfold -- rounded to bf16 (round to nearest even) for the bf16 extractor, unrounded for the fp32 one -- bit for
    bit; the cls row and the pad rows behind the tokens are zero; nothing is written behind the buffer."""
    from dvt_amd.vit import vit_config
    B, img = 2, 48
    c = vit_config(128, 1, patch, stride, img, img, row_pad=32)
    g = (img - patch) // stride + 1
    assert (c.grid_h, c.grid_w, c.n_tokens, c.k_patch) == (g, g, 1 + g * g, 3 * patch * patch) and c.s_pad % 32 == 0
    x = torch.randn(B, 3, img, img, generator=torch.Generator().manual_seed(patch + stride))
    want = torch.zeros(B, c.s_pad, c.k_patch)
    want[:, 1:c.n_tokens] = F.unfold(x, kernel_size=patch, stride=stride).transpose(1, 2)  # [B, g * g, (channel, ky, kx)]
    xd = x.to(DEV)
    n, band = B * c.s_pad * c.k_patch, 4096
    buf = torch.empty(n + band, device=DEV, dtype=torch.int16)
    buf[:n], buf[n:] = NAN16, SENT16
    assert L.dvt_vit_im2col(C.byref(c), xd.data_ptr(), buf.data_ptr(), B, _s()) == 0
    torch.cuda.synchronize()
    assert bool((buf[n:] == SENT16).all()), "bf16 im2col wrote behind its rows"
    got = buf[:n].cpu().view(B, c.s_pad, c.k_patch)
    assert torch.equal(got, want.bfloat16().view(torch.int16)), f"patch {patch} stride {stride}: bf16 im2col differs from unfold"
    buf32 = torch.full((n + band,), float("nan"), device=DEV)
    buf32.view(torch.int32)[n:] = 0x5A5A5A5A
    assert L.dvt_vit_im2col_f32(C.byref(c), xd.data_ptr(), buf32.data_ptr(), B, _s()) == 0
    torch.cuda.synchronize()
    assert bool((buf32.view(torch.int32)[n:] == 0x5A5A5A5A).all()), "fp32 im2col wrote behind its rows"
    assert torch.equal(buf32[:n].cpu().view(B, c.s_pad, c.k_patch), want), f"patch {patch} stride {stride}: fp32 im2col"
    # a grid that does not fit the image is refused before a launch
    bad = vit_config(128, 1, patch, stride, img, img, row_pad=32)
    bad.img_h = img - 1
    assert L.dvt_vit_im2col(C.byref(bad), xd.data_ptr(), buf.data_ptr(), B, _s()) == -1
    assert L.dvt_vit_im2col_f32(C.byref(bad), xd.data_ptr(), buf32.data_ptr(), B, _s()) == -1


# --------------------------------------------------------------------------------------------------------- 2. the forward
def _metrics(got, want):
    d = want.shape[-1]
    cos = F.cosine_similarity(got.double().reshape(-1, d), want.double().reshape(-1, d), dim=-1)
    return float(cos.min()), float((got.double() - want.double()).norm() / want.double().norm())


def hold(got, want, cos_bar, err_bar, what, comparator=None):
    """The bar of tests/test_gpu_vit.py, or -- bf16 only, where it does not hold -- twice the error of `comparator()`, a CPU
    forward of the same arithmetic class against the same float64 reference.  Prints every figure."""
    cmin, err = _metrics(got, want)
    print(f"{what} vs float64 reference: cos min {cmin:.8f} rel-L2 {err:.3e}")
    if cmin > cos_bar and err < err_bar:
        return
    assert comparator is not None, f"{what}: bar (cos > {cos_bar}, rel-L2 < {err_bar}) missed"
    ccmp, ecmp = _metrics(comparator(), want)
    print(f"  bar (cos > {cos_bar}, rel-L2 < {err_bar}) missed; CPU comparator of the same arithmetic class: cos min "
          f"{ccmp:.8f} rel-L2 {ecmp:.3e}")
    assert err <= 2 * ecmp and (1 - cmin) <= 2 * (1 - ccmp), f"{what}: beyond twice the comparator's error"


# (dim, patch, img, stride, LayerScale keys, position table has a cls row, return_cls)
FORWARD_CASES = [
    pytest.param(384, 16, 64, 16, False, 1, False, id="s16-64px-17tok"),
    pytest.param(384, 8, 48, 8, False, 1, False, id="s8-48px-37tok"),
    pytest.param(768, 16, 224, 16, False, 1, False, id="b16-224px-197tok"),
    pytest.param(768, 16, 112, 8, False, 1, False, id="b16-112px-stride8-13x13"),
    pytest.param(768, 16, 64, 16, True, 0, False, id="deit3-layout-64px"),
    pytest.param(768, 8, 48, 8, False, 1, True, id="b8-48px-cls"),
]


@pytest.mark.parametrize("dim,patch,img,stride,ls,cls_row,with_cls", FORWARD_CASES)
def test_forward_two_blocks_vs_reference(L, dim, patch, img, stride, ls, cls_row, with_cls):
    """2 blocks, 2 views, both dtypes, against the float64 reference; the checkpoint grid is the one of stride = patch at this
    image size, so the stride-8 case also resamples the position table.
    MEASURED (one run, one MI355X): DESIGN 13 lists every case."""
    check_forward(dim, patch, img, stride, ls, cls_row, with_cls)


# the token counts the six models produce at their native sizes, and the stride override on patch 16 at 224 (27 x 27)
NATIVE_CASES = [
    pytest.param(768, 16, 384, 16, False, 1, id="b16-384px-577tok"),
    pytest.param(384, 8, 224, 8, False, 1, id="s8-224px-785tok"),
    pytest.param(768, 8, 224, 8, False, 1, id="b8-224px-785tok"),
    pytest.param(768, 16, 224, 8, False, 1, id="b16-224px-stride8-27x27-731tok"),
    pytest.param(768, 16, 112, 8, True, 0, id="deit3-layout-112px-stride8-13x13"),
]


@pytest.mark.parametrize("dim,patch,img,stride,ls,cls_row", NATIVE_CASES)
def test_forward_native_token_counts_vs_reference(L, dim, patch, img, stride, ls, cls_row):
    """2 blocks, ONE view (an odd launch: phantom rows up to a whole 256-row tile), both dtypes, same bars: 577 tokens in 608
    rows, 785 in 800, 731 in 736 with the position table resampled 14 x 14 -> 27 x 27, and the DeiT-III layout (no cls row,
    no registers) with its table resampled 7 x 7 -> 13 x 13 with no prefix row."""
    check_forward(dim, patch, img, stride, ls, cls_row, True, batch=1)


def test_forward_197_tokens_in_256_rows(L, monkeypatch):
    """The product pads 197 tokens to 224 rows; DVT_VIT_ROW_PAD=128 gives the 256 rows the C side's own configuration (and
    the bf16x3 mode) uses: a ragged tail of 59 pad rows per image."""
    monkeypatch.setenv("DVT_VIT_ROW_PAD", "128")
    check_forward(768, 16, 224, 16, False, 1, False, row_pad=128)


def check_forward(dim, patch, img, stride, ls, cls_row, with_cls, batch=2, row_pad=32):
    from dvt_amd.vit import HipViT, random_state_dict
    g0 = img // patch
    g = (img - patch) // stride + 1
    sd = random_state_dict(dim, 2, patch, cls_row + g0 * g0, seed=dim + patch + img, well_conditioned=True, layer_scale=ls)
    assert ("blocks.0.ls1.gamma" in sd) == ls
    x = torch.randn(batch, 3, img, img, generator=torch.Generator().manual_seed(7))
    want, want_cls = bref.forward_features(sd, x, patch, stride, return_cls=True)
    assert want.shape == (batch, g, g, dim)
    tag = f"dim {dim} patch {patch} {img}px stride {stride} ls {ls} pos-cls {cls_row}:"
    cache = {}

    def cmp16(i):
        if "v" not in cache:
            cache["v"] = bref.forward_features(sd, x, patch, stride, return_cls=True, dtype=torch.float32, round_bf16=True)
        return cache["v"][i]

    for dtype, cos_bar, err_bar in (("bfloat16", 0.999, 2e-2), ("float32", 0.999999, 2e-5)):
        vit = HipViT(sd, patch, stride, (img, img), DEV, dtype=dtype)
        c = vit.cfg
        assert (c.patch, c.grid_h, c.grid_w, c.n_prefix, c.pos_has_cls, c.n_tokens) == (patch, g, g, 1, cls_row, 1 + g * g)
        assert c.s_pad == -(-c.n_tokens // row_pad) * row_pad and c.k_patch == 3 * patch * patch
        xd = x.to(DEV)
        if with_cls:
            got, cls = vit.forward_features(xd, return_cls=True)
        else:
            got, cls = vit.forward_features(xd), None
        torch.cuda.synchronize()
        assert got.shape == want.shape and bool(torch.isfinite(got).all())
        comparator = (lambda: cmp16(0)) if dtype == "bfloat16" else None
        hold(got.cpu(), want, cos_bar, err_bar, f"{tag} {dtype} patch tokens", comparator)
        if cls is not None:
            assert cls.shape == (batch, dim)
            hold(cls.cpu(), want_cls, cos_bar, err_bar, f"{tag} {dtype} cls", (lambda: cmp16(1)) if dtype == "bfloat16" else None)
            assert torch.equal(vit.forward_features(xd), got), "the patch tokens depend on return_cls"
        assert torch.equal(vit.forward_features(xd, max_batch=1), got), "the result depends on max_batch"


def test_deit3_position_table_reaches_the_patches_only(L):
    """pos_has_cls = 0 without registers on the device: the engine given the spec's flag and the engine reading the row count
    agree bit for bit, and a table moved by a constant moves the output (it is applied) while the cls output of a 0-block
    forward is LayerNorm(cls_token) alone -- the cls row received no position embedding."""
    from dvt_amd.vit import HipViT, random_state_dict
    dim = 384
    sd = random_state_dict(dim, 1, 16, 9, seed=11, well_conditioned=True)
    x = torch.randn(1, 3, 48, 48, generator=torch.Generator().manual_seed(3)).to(DEV)
    for dtype in ("bfloat16", "float32"):
        a = HipViT(sd, 16, 16, (48, 48), DEV, dtype=dtype, pos_has_cls=0)
        b = HipViT(sd, 16, 16, (48, 48), DEV, dtype=dtype)
        assert a.cfg.pos_has_cls == b.cfg.pos_has_cls == 0
        fa, ca = a.forward_features(x, n_blocks=0, return_cls=True)
        fb, cb = b.forward_features(x, n_blocks=0, return_cls=True)
        assert torch.equal(fa, fb) and torch.equal(ca, cb)
        want_cls = F.layer_norm(sd["cls_token"].double().reshape(1, dim), (dim,), sd["norm.weight"].double(),
                                sd["norm.bias"].double(), 1e-6)
        torch.testing.assert_close(ca.cpu().double(), want_cls, rtol=1e-5, atol=1e-5)
        moved = HipViT(dict(sd, pos_embed=sd["pos_embed"] + 0.5 * torch.randn(1, 9, dim, generator=torch.Generator().manual_seed(1))), 16, 16, (48, 48), DEV, dtype=dtype)
        fm, cm = moved.forward_features(x, n_blocks=0, return_cls=True)
        assert torch.equal(cm, ca) and not torch.equal(fm, fa)


def test_vitb16_dino_full_depth(L):
    """`vit_base_patch16_224.dino` through the wrapper at FULL depth: 12 blocks, 224 x 224 (197 tokens), 1 view, well-conditioned
    random weights, both dtypes, against the float64 reference.  Bars: the full-depth ViT-B bar of tests/test_gpu_vit.py for
    bf16 (per-token cosine min > 0.999), the fp32 bars of the same file (rel-L2 < 2e-5, cosine > 0.999999).
    MEASURED (one run, one MI355X): DESIGN 13 lists every case."""
    from dvt_amd.models import PretrainedViTWrapper
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = PretrainedViTWrapper("vit_base_patch16_224.dino", stride=16, allow_random_init=True)
    assert (w.n_output_dims, w.num_blocks, w.patch_size) == (768, 12, 16)
    sd = w._state_dict
    x = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(5))
    want = bref.forward_features(sd, x, 16, 16)
    assert want.shape == (1, 14, 14, 768) and bool(torch.isfinite(want).all())
    got = w.get_intermediate_layers(x.to(DEV), n=[11], reshape=True)[0].permute(0, 2, 3, 1).cpu()
    cmin, err = _metrics(got, want)
    print(f"ViT-B/16 DINO layout FULL depth bf16 vs float64 reference: cos min {cmin:.8f} rel-L2 {err:.3e}")
    if not cmin > 0.999:
        ccmp, ecmp = _metrics(bref.forward_features(sd, x, 16, 16, dtype=torch.float32, round_bf16=True), want)
        print(f"  bar (cos > 0.999) missed; CPU comparator of the same arithmetic class: cos min {ccmp:.8f} rel-L2 {ecmp:.3e}")
        assert (1 - cmin) <= 2 * (1 - ccmp) and err <= 2 * ecmp
    got32 = w.features_nhwc(x.to(DEV), dtype="float32").cpu()
    hold(got32, want, 0.999999, 2e-5, "ViT-B/16 DINO layout FULL depth fp32")


# --------------------------------------------------------------------------------------------------- 3. stage 1 end to end
def test_stage1_cli_vit_small_patch16_dino(L, tmp_path):
    """`python -m dvt_amd.stage1 --model vit_small_patch16_224.dino --synthetic ...` in a child process under its own time
    limit: both outputs exist, 14 x 14 x 384, finite; the raw features are the extractor's on the same (last, whole-image)
    view -- the same fp32 kernels, so to fp32 round-off (the fp32 forward bar, 2e-5)."""
    from dvt_amd import views as V
    from dvt_amd.models import PretrainedViTWrapper
    model = "vit_small_patch16_224.dino"
    (tmp_path / "data").mkdir()
    (tmp_path / "list.txt").write_text("a.png\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "denoising-vit_amd"), ROOT]))
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "dvt_amd.stage1", "--model", model, "--synthetic",
           "--allow_random_vit", "--num_imgs", "1", "--input_size", "224", "--stride_size", "16", "--num_views", "7",
           "--num_iters", "40", "--warmup_iters", "4", "--pixel_bsz", "512", "--seed", "3", "--img_path",
           str(tmp_path / "list.txt"), "--data_root", str(tmp_path / "data"), "--save_root", str(tmp_path / "out"),
           "--output_dir", str(tmp_path / "work")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    raw = np.load(tmp_path / "out" / "raw_features" / model / "a.npy")
    den = np.load(tmp_path / "out" / "denoised_features" / model / "a.npy")
    assert raw.shape == (14, 14, 384) and raw.dtype == np.float32 and den.shape == (1, 14, 14, 384)
    assert np.isfinite(raw).all() and np.isfinite(den).all() and np.abs(den).max() > 0
    views, _ = V.synthetic_views(7, (224, 224), 14, 14, torch.device(DEV), seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = PretrainedViTWrapper(model, stride=16, img_size=(224, 224), allow_random_init=True, dtype="float32")
    direct = w.features_nhwc(views[-1:], w.last_layer_index).cpu()[0]
    err = float((torch.from_numpy(raw) - direct).norm() / direct.norm())
    print(f"stage 1 raw features vs a direct features_nhwc call on the same view: rel-L2 {err:.3e}")
    assert err < 2e-5
