"""GPU: the opt-in bf16 inference forward of the stage-2 Denoiser (csrc/dvt_denoiser.hip, dvt_amd/denoiser_bf16.py) -- the
stand-alone forward against the float64 reference of tests/denoiser_reference.py at the edges of its tiling, another grid than
the noise map's and the cache's invalidation, the fused image-in forward bit for bit against the composition of the
extractor and the stand-alone forward, sentinel bands behind every output, every refusal, and the untouched float32 default.

Bars (none of them comes from what the code under test gives): those of tests/test_gpu_vit.py as tests/test_gpu_backbones.py
uses them -- bf16 per-token cosine min > 0.999 and rel-L2 < 2e-2 against the float64 reference; where a case misses them,
`hold` computes a CPU forward of the same arithmetic class (every matrix operand rounded to bf16) against the same reference
and allows twice ITS error.
"""
import ctypes as C
import warnings

import pytest
import torch
import torch.nn.functional as F

from tests import denoiser_reference as dref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAND = 4096
SENT = 0x5A5A5A5A


def _s():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def L(built_lib):
    import dvt_amd.denoiser_bf16  # noqa: F401 registers signatures
    return built_lib


def _metrics(got, want):
    d = want.shape[-1]
    cos = F.cosine_similarity(got.double().reshape(-1, d), want.double().reshape(-1, d), dim=-1)
    return float(cos.min()), float((got.double() - want.double()).norm() / want.double().norm())


def hold(got, want, cos_bar, err_bar, what, comparator=None):
    """The bar of tests/test_gpu_vit.py, or -- bf16 only, where it does not hold -- twice the error of `comparator()`, a CPU
    forward of the same arithmetic class against the same float64 reference.  Prints every figure.  (tests/test_gpu_backbones.py)"""
    cmin, err = _metrics(got, want)
    print(f"{what} vs float64 reference: cos min {cmin:.8f} rel-L2 {err:.3e}")
    if cmin > cos_bar and err < err_bar:
        return
    assert comparator is not None, f"{what}: bar (cos > {cos_bar}, rel-L2 < {err_bar}) missed"
    ccmp, ecmp = _metrics(comparator(), want)
    print(f"  bar (cos > {cos_bar}, rel-L2 < {err_bar}) missed; CPU comparator of the same arithmetic class: cos min "
          f"{ccmp:.8f} rel-L2 {ecmp:.3e}")
    assert err <= 2 * ecmp and (1 - cmin) <= 2 * (1 - ccmp), f"{what}: beyond twice the comparator's error"


def banded(n):
    """n floats of NaN with a sentinel band behind them."""
    buf = torch.full((n + BAND,), float("nan"), device=DEV)
    buf.view(torch.int32)[n:] = SENT
    return buf


def band_intact(buf, n):
    return bool((buf.view(torch.int32)[n:] == SENT).all())


def filled_workspace(nbytes, fill):
    assert nbytes > 0
    if fill == "zeros":
        return torch.zeros(nbytes, device=DEV, dtype=torch.uint8)
    ws = torch.empty(nbytes // 4 + 1, device=DEV)
    ws.fill_(float("nan"))
    return ws


def run_alone(L, hd, feats, fill="nan"):
    """dvt_denoiser_forward_bf16 through the C ABI on a workspace of the test's own; -> (out, band intact)."""
    B, n = feats.shape[0], feats.numel()
    ws = filled_workspace(L.dvt_denoiser_workspace_bytes(C.byref(hd.cfg), B), fill)
    buf = banded(n)
    feats = feats.contiguous()
    assert L.dvt_denoiser_forward_bf16(C.byref(hd.cfg), C.byref(hd.weights), feats.data_ptr(), buf.data_ptr(), B, ws.data_ptr(),
                                       _s()) == 0
    torch.cuda.synchronize()
    return buf[:n].view(feats.shape).clone(), band_intact(buf, n)


# ---------------------------------------------------------------------------------------------- 1. the stand-alone forward
# (dim, grid, batch, num_blocks, enable_pe)
ALONE_CASES = [
    pytest.param(768, (5, 5), 2, 1, True, id="768-5x5-b2"),             # 25 tokens in 32 rows, half a key tile
    pytest.param(768, (8, 8), 1, 1, True, id="768-8x8-b1"),             # 64 = s_pad, no masked key, odd batch, phantom rows
    pytest.param(768, (5, 13), 3, 2, True, id="768-5x13-b3-2blocks"),   # 65 tokens in 96 rows, one key in the last tile
    pytest.param(384, (6, 6), 2, 1, False, id="384-6x6-b2-no-pe"),      # unfolded LayerNorm path, no pos_embed
    pytest.param(1024, (7, 7), 1, 1, True, id="1024-7x7-b1"),
    pytest.param(768, (37, 37), 1, 1, True, id="768-37x37-b1"),         # the native grid, once
]


@pytest.mark.parametrize("dim,grid,batch,num_blocks,enable_pe", ALONE_CASES)
def test_forward_vs_reference(L, dim, grid, batch, num_blocks, enable_pe):
    """dvt_denoiser_forward_bf16 against the float64 reference; LayerNorm-like features, pos_embed of scale 0.02,
    well-conditioned random weights.  The output's sentinel band is intact; a zero-filled and a NaN-filled workspace give the
    same bits.
    MEASURED (one run, one MI355X): DESIGN 17 lists every case."""
    from dvt_amd.denoiser_bf16 import HipDenoiser
    sd = dref.random_denoiser_state(dim, num_blocks, grid, seed=dim + grid[0] * grid[1], enable_pe=enable_pe)
    feats = dref.layernorm_like_features(batch, grid, dim, seed=5)
    want = dref.forward(sd, feats, num_blocks)
    hd = HipDenoiser(sd, grid, grid, num_blocks, enable_pe, DEV)
    assert hd.cfg.s_pad == -(-grid[0] * grid[1] // 32) * 32 and hd.cfg.n_tokens == grid[0] * grid[1]
    got, intact = run_alone(L, hd, feats.to(DEV), "nan")
    assert intact, "dvt_denoiser_forward_bf16 wrote behind out"
    assert bool(torch.isfinite(got).all())
    what = f"denoiser bf16 dim {dim} grid {grid[0]}x{grid[1]} batch {batch} blocks {num_blocks} pe {enable_pe}:"
    hold(got.cpu(), want, 0.999, 2e-2, what, lambda: dref.forward(sd, feats, num_blocks, dtype=torch.float32, round_bf16=True))
    got0, _ = run_alone(L, hd, feats.to(DEV), "zeros")
    assert torch.equal(got0, got), "the result depends on what the workspace held"
    assert torch.equal(hd.forward(feats.to(DEV)), got), "HipDenoiser.forward differs from the C entry point"
    if batch > 1:  # (results do not depend on how images are batched)
        assert torch.equal(hd.forward(feats[:1].to(DEV)), got[:1])


# ------------------------------------------------------------------------------- 2. a grid other than the noise map's
def test_denoiser_module_other_grid_and_cache_invalidation(L):
    """Denoiser(noise map 8 x 8, inference_dtype="bfloat16") on 5 x 13 features equals the reference fed the resampled
    position table, at the same bars; after a parameter change through the engine (load_named) the next forward is the new
    parameters' (the bf16 weights are dropped with engine.param_version)."""
    from dvt_amd.models.online_denoiser import Denoiser
    dim, grid = 768, (5, 13)
    sd = dref.random_denoiser_state(dim, 1, (8, 8), seed=21)
    den = Denoiser(8, 8, dim, device=DEV, seed=0, inference_dtype="bfloat16")
    den.load_state_dict(sd)
    feats = dref.layernorm_like_features(2, grid, dim, seed=6)
    cmp16 = lambda s: (lambda: dref.forward(s, feats, noise_map=(8, 8), dtype=torch.float32, round_bf16=True))  # noqa: E731
    got = den(feats.to(DEV))
    assert got.shape == feats.shape and list(den._bf16) == [grid]
    hold(got.cpu(), dref.forward(sd, feats, noise_map=(8, 8)), 0.999, 2e-2, "Denoiser bf16 8x8 table on 5x13 features:", cmp16(sd))
    assert torch.equal(den(feats.to(DEV)), got)
    sd2 = dict(sd)
    g = torch.Generator().manual_seed(1)
    sd2["denoiser.attn.proj.bias"] = sd["denoiser.attn.proj.bias"] + torch.randn(dim, generator=g)
    sd2["pos_embed"] = sd["pos_embed"] + 0.02 * torch.randn(1, 64, dim, generator=g)
    version = den.engine.param_version
    den.engine.load_named(sd2)
    assert den.engine.param_version == version + 1
    got2 = den(feats.to(DEV))
    assert not torch.equal(got2, got)
    hold(got2.cpu(), dref.forward(sd2, feats, noise_map=(8, 8)), 0.999, 2e-2, "... after load_named:", cmp16(sd2))
    # the LRU cap of the resized fp32 copies holds for the bf16 weights too
    for g_ in ((4, 4), (4, 5), (4, 6), (4, 7), (4, 8)):
        den(dref.layernorm_like_features(1, g_, dim).to(DEV))
    assert len(den._bf16) == Denoiser.RESIZED_CACHE and grid not in den._bf16


# ------------------------------------------------------------------------------------- 3. + 4. the fused forward
def run_fused(L, hd, vit, img, fill, want_orig=True, want_cls=True):
    """dvt_vit_forward_denoised through the C ABI on a workspace of the test's own; -> (out, orig, cls, bands intact)."""
    B, vc, dc = img.shape[0], vit.cfg, hd.cfg
    n, ncls = B * dc.n_tokens * dc.dim, B * dc.dim
    ws = filled_workspace(L.dvt_vit_workspace_bytes_denoised(C.byref(vc), C.byref(dc), B), fill)
    out, orig, cls = banded(n), banded(n), banded(ncls)
    rc = L.dvt_vit_forward_denoised(C.byref(vc), C.byref(vit.weights), C.byref(dc), C.byref(hd.weights), img.data_ptr(),
                                    out.data_ptr(), orig.data_ptr() if want_orig else None, cls.data_ptr() if want_cls else None,
                                    B, ws.data_ptr(), _s())
    assert rc == 0
    torch.cuda.synchronize()
    shape = (B, dc.grid_h, dc.grid_w, dc.dim)
    return (out[:n].view(shape).clone(), orig[:n].view(shape).clone(), cls[:ncls].view(B, dc.dim).clone(),
            band_intact(out, n) and band_intact(orig, n) and band_intact(cls, ncls))


# (dim, patch, (img_h, img_w), register tokens): n_prefix = 1 + registers
FUSED_CASES = [
    pytest.param(768, 16, (64, 64), 0, id="768-p16-64px-4x4"),   # n_prefix 1
    pytest.param(768, 14, (70, 70), 4, id="768-reg4-5x5"),       # rows move by 5 prefix rows (30 tokens, 25 patches: 32 rows each)
    pytest.param(768, 16, (80, 96), 4, id="768-reg4-5x6"),       # 35 tokens in 64 rows, 30 patches in 32: s_pad2 < s_pad
    pytest.param(384, 16, (64, 64), 0, id="384-p16-64px-4x4"),   # the unfolded path
]


@pytest.mark.parametrize("dim,patch,img,n_reg", FUSED_CASES)
def test_fused_equals_composition_bit_for_bit(L, dim, patch, img, n_reg):
    """A 2-block ViT + a 1-block denoiser: dvt_vit_forward_denoised's original_feats are forward_features' bits, its cls those
    of return_cls=True, its out the bits of dvt_denoiser_forward_bf16 on those features -- at batch 1 and 3, on a zero-filled
    and a NaN-filled workspace, with the sentinel band behind out, original_feats and cls intact, with and without the two
    optional outputs.  (The 5 x 5 register case pads 30 tokens and 25 patches to 32 rows each; the 5 x 6 one is the layout in
    which the denoiser's images are SHORTER than the extractor's, 32 rows against 64.)"""
    from dvt_amd.denoiser_bf16 import HipDenoiser
    from dvt_amd.vit import HipViT, random_state_dict
    g0 = img[0] // patch
    grid = (img[0] // patch, img[1] // patch)
    vsd = random_state_dict(dim, 2, patch, (0 if n_reg else 1) + g0 * g0, seed=dim + n_reg, well_conditioned=True, n_reg=n_reg)
    vit = HipViT(vsd, patch, patch, img, DEV)
    hd = HipDenoiser(dref.random_denoiser_state(dim, 1, grid, seed=3), grid, grid, 1, True, DEV)
    vc, dc = vit.cfg, hd.cfg
    assert (vc.grid_h, vc.grid_w, vc.n_prefix) == (*grid, 1 + n_reg) and dc.s_pad <= vc.s_pad
    if grid == (5, 6):
        assert (vc.s_pad, dc.s_pad) == (64, 32)
    for batch in (1, 3):
        x = torch.randn(batch, 3, *img, generator=torch.Generator().manual_seed(batch)).to(DEV)
        feat, cls = vit.forward_features(x, return_cls=True)
        want, _ = run_alone(L, hd, feat, "nan")
        for fill in ("zeros", "nan"):
            out, orig, c, intact = run_fused(L, hd, vit, x, fill)
            assert intact, f"batch {batch} {fill}: the fused forward wrote behind an output"
            assert torch.equal(orig, feat), f"batch {batch} {fill}: original_feats differ from forward_features"
            assert torch.equal(c, cls), f"batch {batch} {fill}: cls differs from forward_features(return_cls=True)"
            assert torch.equal(out, want), f"batch {batch} {fill}: out differs from the stand-alone forward on those features"
        out, orig, c, intact = run_fused(L, hd, vit, x, "nan", want_orig=False, want_cls=False)
        assert intact and torch.equal(out, want) and bool(torch.isnan(orig).all()) and bool(torch.isnan(c).all())
        o2, f2, c2 = hd.forward_fused(vit, x, return_original=True, return_cls=True)
        assert torch.equal(o2, want) and torch.equal(f2, feat) and torch.equal(c2, cls)
        assert torch.equal(vit.forward_features(x), feat), "the extractor's own forward changed after the fused call"


# ----------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_before_any_launch(L):
    """Every DVT_E_BADARG case of include/dvt_denoiser.h returns -1 with the outputs still holding their fill."""
    from dvt_amd.denoiser_bf16 import DenoiserWeights, HipDenoiser
    from dvt_amd.vit import HipViT, VitWeights, random_state_dict
    dim, grid = 768, (4, 4)
    hd = HipDenoiser(dref.random_denoiser_state(dim, 1, grid, seed=3), grid, grid, 1, True, DEV)
    vit = HipViT(random_state_dict(dim, 2, 16, 17, seed=1, well_conditioned=True), 16, 16, (64, 64), DEV)
    B, n = 2, 2 * 16 * dim
    feats = dref.layernorm_like_features(B, grid, dim).to(DEV)
    img = torch.randn(B, 3, 64, 64, device=DEV)
    ws = torch.zeros(L.dvt_vit_workspace_bytes_denoised(C.byref(vit.cfg), C.byref(hd.cfg), B), device=DEV, dtype=torch.uint8)
    out, orig, cls = banded(n), banded(n), banded(B * dim)

    def cfg(**kw):
        c = type(hd.cfg).from_buffer_copy(hd.cfg)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def weights(**kw):
        w = DenoiserWeights.from_buffer_copy(hd.weights)
        for k, v in kw.items():
            if k == "pos_embed":
                w.pos_embed = v
            else:
                setattr(w.blocks[0], k, v)
        return w

    bad_cfgs = [cfg(dim=512, heads=8, mlp_dim=2048), cfg(dim=1536, heads=24, mlp_dim=6144), cfg(heads=11), cfg(mlp_dim=2048),
                cfg(n_tokens=15), cfg(grid_h=5), cfg(s_pad=48), cfg(s_pad=0), cfg(n_blocks=0), cfg(n_blocks=9), cfg(ln_eps=0.0)]
    bad_ws = [weights(pos_embed=None), weights(qkv_w=None), weights(fc2_b=None), weights(ls1=None), weights(fc1_cs=None)]

    def alone(c=hd.cfg, w=hd.weights, f=feats.data_ptr(), o=out.data_ptr(), b=B, k=ws.data_ptr()):
        return L.dvt_denoiser_forward_bf16(C.byref(c) if c is not None else None, C.byref(w) if w is not None else None, f, o, b, k, _s())

    def fused(vc=vit.cfg, vw=vit.weights, c=hd.cfg, w=hd.weights, i=img.data_ptr(), o=out.data_ptr(), b=B, k=ws.data_ptr()):
        return L.dvt_vit_forward_denoised(C.byref(vc) if vc is not None else None, C.byref(vw) if vw is not None else None,
                                          C.byref(c) if c is not None else None, C.byref(w) if w is not None else None, i, o,
                                          orig.data_ptr(), cls.data_ptr(), b, k, _s())

    for c in bad_cfgs:
        assert alone(c=c) == -1 and fused(c=c) == -1, [getattr(c, f[0]) for f in c._fields_]
    for w in bad_ws:
        assert alone(w=w) == -1 and fused(w=w) == -1
    for kw in (dict(c=None), dict(w=None), dict(f=None), dict(o=None), dict(k=None), dict(b=0), dict(b=-1)):
        assert alone(**kw) == -1, kw
    for kw in (dict(vc=None), dict(vw=None), dict(c=None), dict(w=None), dict(i=None), dict(o=None), dict(k=None), dict(b=0)):
        assert fused(**kw) == -1, kw
    # the extractor's side: what dvt_vit_forward refuses, a final norm that is missing, a geometry that is not the denoiser's
    vbad = type(vit.cfg).from_buffer_copy(vit.cfg)
    vbad.n_prefix, vbad.n_tokens = 0, 16
    assert fused(vc=vbad) == -1
    vnn = VitWeights.from_buffer_copy(vit.weights)
    vnn.norm_w = None
    assert fused(vw=vnn) == -1
    other = HipDenoiser(dref.random_denoiser_state(dim, 1, (5, 5), seed=3), (5, 5), (5, 5), 1, True, DEV)
    assert fused(c=other.cfg, w=other.weights) == -1
    assert fused(c=cfg(s_pad=64)) == -1  # longer images than the extractor's
    torch.cuda.synchronize()
    for buf, m in ((out, n), (orig, n), (cls, B * dim)):
        assert bool(torch.isnan(buf[:m]).all()) and band_intact(buf, m), "a refused call wrote to an output"
    assert alone() == 0 and fused() == 0  # (and the good arguments run)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:n]).all())


# ----------------------------------------------------------------------------------------- 6. + 7. the Denoiser module
def _wrapper(dtype):
    from dvt_amd.models import PretrainedViTWrapper
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return PretrainedViTWrapper("vit_base_patch16_224.dino", stride=16, img_size=64, allow_random_init=True, dtype=dtype)


def test_float32_default_is_untouched(L):
    """inference_dtype="float32" (the default): Denoiser.forward is Stage2Engine.forward bit for bit, without a vit and with
    one; a float32 wrapper under inference_dtype="bfloat16" is refused by name, and so is norm=False."""
    from dvt_amd.models.online_denoiser import Denoiser
    dim = 768
    sd = dref.random_denoiser_state(dim, 1, (4, 4), seed=8)
    den = Denoiser(4, 4, dim, device=DEV, seed=0)
    assert den.inference_dtype == "float32"
    den.load_state_dict(sd)
    feats = dref.layernorm_like_features(2, (4, 4), dim, seed=2).to(DEV)
    want = den.engine.forward(feats.reshape(2, 16, dim)).reshape(2, 4, 4, dim)
    assert torch.equal(den(feats), want) and not den._bf16
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(4)).to(DEV)
    for dtype in ("bfloat16", "float32"):
        w = _wrapper(dtype)
        dv = Denoiser(4, 4, dim, vit=w, device=DEV, seed=0, inference_dtype="float32")
        dv.load_state_dict(sd)
        f = w.features_nhwc(x)
        res = dv(x, return_dict=True, return_class_token=True)
        assert torch.equal(res["original_feats"], f)
        assert torch.equal(res["denoised_feats"], dv.engine.forward(f.reshape(2, 16, dim).contiguous()).reshape(2, 4, 4, dim))
        assert not dv._bf16
    with pytest.raises(ValueError, match="float32"):
        Denoiser(4, 4, dim, vit=_wrapper("float32"), device=DEV, inference_dtype="bfloat16")
    with pytest.raises(ValueError, match="norm=False"):
        Denoiser(4, 4, dim, vit=_wrapper("bfloat16"), device=DEV, inference_dtype="bfloat16")(x, norm=False)


def test_denoiser_module_over_a_bf16_wrapper(L):
    """Denoiser(vit=bf16 wrapper, inference_dtype="bfloat16") at 64 px / patch 16: return_dict returns the three keys with the
    fused call's bits -- original_feats the wrapper's features, class_tokens its cls token, denoised_feats the stand-alone
    bf16 forward on those features -- return_channel_first permutes, and the tuple / plain forms return the same tensors."""
    from dvt_amd.models.online_denoiser import Denoiser
    dim = 768
    w = _wrapper("bfloat16")
    den = Denoiser(4, 4, dim, vit=w, device=DEV, seed=0, inference_dtype="bfloat16")
    sd = dref.random_denoiser_state(dim, 1, (4, 4), seed=8)
    den.load_state_dict(sd)
    x = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(4)).to(DEV)
    res = den(x, return_dict=True, return_class_token=True)
    assert sorted(res) == ["class_tokens", "denoised_feats", "original_feats"]
    feat, cls = w.features_nhwc(x, return_cls=True)
    hd = den._bf16_for(4, 4)
    assert torch.equal(res["original_feats"], feat) and torch.equal(res["class_tokens"], cls)
    assert torch.equal(res["denoised_feats"], hd.forward(feat))
    o, f, c = hd.forward_fused(w._engine(x.device), x, return_original=True, return_cls=True)
    assert torch.equal(o, res["denoised_feats"]) and torch.equal(f, feat) and torch.equal(c, cls)
    hold(res["denoised_feats"].cpu(), dref.forward(sd, feat.cpu()), 0.999, 2e-2, "Denoiser over a bf16 wrapper, on its features:",
         lambda: dref.forward(sd, feat.cpu(), dtype=torch.float32, round_bf16=True))
    chw = den(x, return_dict=True, return_channel_first=True)
    assert chw["class_tokens"] is None and torch.equal(chw["denoised_feats"], res["denoised_feats"].permute(0, 3, 1, 2))
    assert torch.equal(chw["original_feats"], feat)
    y, ct = den(x, return_class_token=True)
    assert torch.equal(y, res["denoised_feats"]) and torch.equal(ct, cls)
    assert torch.equal(den(x), res["denoised_feats"])
