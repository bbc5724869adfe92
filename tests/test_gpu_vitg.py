"""GPU: the ViT-g/14 backbone -- the SwiGLU fc1 epilogue element by element against fp64, the width-1536 row kernels, the
forward of the giant geometry against tests/vitg_reference.py (float64), and the unchanged bits of the existing models.

Bounds (none of them comes from what the code under test gives):
  * SwiGLU epilogue: the fp32 values g (gate) and v (value) carry the accumulation bounds of test_gpu_vit_epilogues.py
    (K 2^-24 sum |a| |w|, plus the fold's fp32 correction).  With |silu'| <= 1.1 the product silu(g) v is off by at most
    1.1 |v| bound_g + |silu(g)| bound_v; the kernel's silu (v_exp_f32 of g log2 e, v_rcp_f32: 1 ulp each, the exponent's
    argument rounded once) adds (|g| 2^-22 + 2^-20) |silu(g) v|; the bf16 store 2^-8 relative.
  * LayerNorm statistics at 1536: the bounds test_ln_cast_stats_vs_fp64 uses at 1024.
  * Whole forward: the project's bars of test_vit_large_full_depth (bf16: per-token cosine > 0.999, rel-L2 < 3e-2; fp32:
    rel-L2 <= 1e-5, cosine > 0.999999).  Those were observed on the GELU models.  Where one does not hold, `hold` computes a
    CPU forward of the same arithmetic class (fp32: torch fp32; bf16: the fp32 forward with every matrix operand and stored
    activation rounded to bf16) against the same float64 reference and allows twice ITS error.
"""
import ctypes as C
import json
import os
import warnings

import pytest
import torch
import torch.nn.functional as F

from tests import vitg_reference as vref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BADARG = -1
GEMM_DEFAULT = 4
U = 2.0 ** -24
NAN16, SENT16 = 0x7FC0, 0x5A5A
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vitb_2block_parent.json")


def _s():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def L(built_lib):
    import dvt_amd.vit  # noqa: F401 registers signatures
    return built_lib


def gemm_schedule(L, v):
    class _Sched:
        def __enter__(self):
            assert L.dvt_tune_set(1, v) == 0

        def __exit__(self, *exc):
            assert L.dvt_tune_set(1, GEMM_DEFAULT) == 0
    return _Sched()


def banded16(n, band):
    buf = torch.empty(n + band, device=DEV, dtype=torch.int16)
    buf[:n] = NAN16
    buf[n:] = SENT16
    return buf[:n].view(torch.bfloat16), buf[n:], buf


def banded32(n, band):
    buf = torch.full((n + band,), float("nan"), device=DEV, dtype=torch.float32)
    buf.view(torch.int32)[n:] = 0x5A5A5A5A
    return buf[:n], buf.view(torch.int32)[n:], buf


def assert_band(band, pattern, what):
    bad = (band != pattern).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.numel()} sentinel elements overwritten, first at band offset {int(bad[0])}"


def assert_close(got, ref, tol, what):
    got = got.double()
    err = (got - ref).abs()
    bad = ~(err <= tol)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements out of tolerance; first at {idx}: "
                             f"got {float(got.flatten()[i])!r} want {float(ref.flatten()[i])!r} tol {float(tol.flatten()[i]):.3g}")


def bf16_tol(ref, acc):
    return 2.0 ** -8 * ref.abs() + 2.0 * acc + 2.0 ** -22 * ref.abs() + 1e-30


def acc_bound(a, w):
    return a.shape[1] * U * (a.double().abs() @ w.double().abs().t())


def rand_bf16(*shape, gen, scale=1.0):
    return (torch.randn(*shape, generator=gen, device=DEV) * scale).bfloat16()


# ------------------------------------------------------------------------------------------------- 1. the SwiGLU epilogue
@pytest.mark.parametrize("variant", [1, 3, 4])
@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("m,hid,k", [(512, 4096, 1536), (256, 64, 128)])
def test_swiglu_epilogue_vs_fp64(L, m, hid, k, fold, variant):
    """dvt_vit_gemm_swiglu: y[m, j] = silu(g_j) v_j from the PACKED weights (packed here, from a plain [2 H, K] matrix, with
    the documented permutation), folded and plain, per element against fp64; gates of +-100 and +-60 (bias) stay finite.
    The folded form on the 128 x 128 schedule is refused with the output untouched."""
    from dvt_amd.vit import swiglu_pack
    g = torch.Generator(device=DEV).manual_seed(m + hid + k + 10 * fold)
    w = rand_bf16(2 * hid, k, gen=g, scale=2.0 / k ** 0.5)
    w[:, :8] += 0.05
    b = torch.randn(2 * hid, generator=g, device=DEV) * 0.5
    b[:8] = torch.tensor([100.0, -100.0, 60.0, -60.0, 30.0, -30.0, 88.0, -88.0], device=DEV)  # gate range: |g| up to ~100
    b[hid - 4:hid] = torch.tensor([120.0, -120.0, 100.0, -100.0], device=DEV)                   # ... and in the last block
    xf = torch.randn(m, k, generator=g, device=DEV) * (0.5 + torch.rand(m, 1, generator=g, device=DEV) * 2)
    xf += torch.randn(m, 1, generator=g, device=DEV) * 3
    x = xf.bfloat16()
    acc = x.double() @ w.double().t()
    bound = acc_bound(x, w)
    st = cs = None
    if fold:
        x64 = xf.double()
        st = torch.stack([x64.mean(1), 1.0 / torch.sqrt(x64.var(1, unbiased=False) + 1e-6)], 1).float().contiguous()
        cs = w.float().sum(1).contiguous()
        mu, rs = st[:, 0:1].double(), st[:, 1:2].double()
        v = rs * (acc - mu * cs.double()) + b.double()
        bound = rs * (bound + 4 * U * (acc.abs() + (mu * cs.double()).abs())) + 2 * U * v.abs()
    else:
        v = acc + b.double()
    gate, val = v[:, :hid], v[:, hid:]
    silu = gate * torch.sigmoid(gate)
    ref = silu * val
    err = 1.1 * val.abs() * bound[:, :hid] + silu.abs() * bound[:, hid:] + (gate.abs() * 2.0 ** -22 + 2.0 ** -20) * ref.abs()
    assert float(gate.abs().max()) > 95.0  # the range the issue asks for is really there
    wp, bp = swiglu_pack(w).contiguous(), swiglu_pack(b).contiguous()
    csp = swiglu_pack(cs).contiguous() if fold else None
    y, band, _ = banded16(m * hid, 4096)
    with gemm_schedule(L, variant):
        rc = L.dvt_vit_gemm_swiglu(x.data_ptr(), wp.data_ptr(), bp.data_ptr(), y.data_ptr(), m, hid, k,
                                   st.data_ptr() if fold else None, csp.data_ptr() if fold else None, _s())
        torch.cuda.synchronize()
    if fold and variant == 1:
        assert rc == BADARG and bool(y.isnan().all())
        assert_band(band, SENT16, "swiglu band (refused)")
        return
    assert rc == 0
    assert_band(band, SENT16, "swiglu band")
    assert bool(torch.isfinite(y.float()).all()), "silu(g) * v is not finite somewhere"
    assert_close(y.view(m, hid), ref, bf16_tol(ref, err), f"swiglu fold={fold} schedule={variant}")


def test_swiglu_rejects_misaligned_before_writing(L):
    m, hid, k = 256, 128, 128
    x = torch.zeros(m, k, device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(2 * hid, k, device=DEV, dtype=torch.bfloat16)
    b = torch.zeros(2 * hid, device=DEV)
    st = torch.zeros(m, 2, device=DEV)
    y, band, _ = banded16(m * hid, 1024)
    call = lambda m_, h_, k_, st_=None, cs_=None: L.dvt_vit_gemm_swiglu(  # noqa: E731
        x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), m_, h_, k_, st_, cs_, _s())
    assert call(100, hid, k) == BADARG and call(m, 96, k) == BADARG and call(m, hid, 96) == BADARG
    assert call(m, hid, k, st.data_ptr(), None) == BADARG  # stats without column sums
    assert call(128, hid, k, st.data_ptr(), b.data_ptr()) == BADARG  # folded: whole 256-row tiles
    torch.cuda.synchronize()
    assert bool(y.isnan().all())
    assert_band(band, SENT16, "band")


def test_unfused_swiglu_equals_reference(L):
    """dvt_vit_swiglu_act (the A/B's unfused form): silu(g) * v on a full-width bf16 row, one bf16 rounding."""
    m, hid = 64, 256
    g = torch.Generator(device=DEV).manual_seed(3)
    h = (torch.randn(m, 2 * hid, generator=g, device=DEV) * 4).bfloat16()
    h[0, :4] = torch.tensor([100.0, -100.0, 60.0, -60.0], device=DEV).bfloat16()
    out, band, _ = banded16(m * hid, 512)
    assert L.dvt_vit_swiglu_act(h.data_ptr(), out.data_ptr(), m, hid, _s()) == 0
    torch.cuda.synchronize()
    assert_band(band, SENT16, "band")
    gt, vl = h[:, :hid].double(), h[:, hid:].double()
    ref = gt * torch.sigmoid(gt) * vl
    assert_close(out.view(m, hid), ref, bf16_tol(ref, (gt.abs() * 2.0 ** -22 + 2.0 ** -20) * ref.abs()), "swiglu_act")


# ------------------------------------------------------------------------------------------- 2. row kernels at width 1536
def stat_rows(rows, dim, gen):
    x = torch.randn(rows, dim, generator=gen, device=DEV)
    kind = torch.arange(rows, device=DEV) % 4
    x[kind == 1] = x[kind == 1] + 1e3
    x[kind == 2] = x[kind == 2] * 0.01 - 5
    x[kind == 3] = x[kind == 3] * 100
    return x.contiguous()


@pytest.mark.parametrize("rows,dim", [(301, 1536), (97, 1280), (4352, 1536)])
def test_ln_cast_stats_1536_vs_fp64(L, rows, dim):
    eps = 1e-6
    x = stat_rows(rows, dim, torch.Generator(device=DEV).manual_seed(rows + dim))
    xb, xb_band, _ = banded16(rows * dim, 2048)
    st, st_band, _ = banded32(rows * 2, 256)
    assert L.dvt_vit_ln_cast_stats(x.data_ptr(), xb.data_ptr(), st.data_ptr(), rows, dim, C.c_float(eps), _s()) == 0
    torch.cuda.synchronize()
    assert_band(xb_band, SENT16, "xb band")
    assert_band(st_band, 0x5A5A5A5A, "stats band")
    assert torch.equal(xb.view(rows, dim).view(torch.int16), x.bfloat16().view(torch.int16)), "xb is not bf16(x)"
    x64 = x.double()
    mean, var = x64.mean(1), x64.var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    st = st.view(rows, 2).double()
    assert_close(st[:, 0], mean, 2.0 ** -18 * x64.abs().mean(1), "mean")
    assert_close(st[:, 1] / rstd, torch.ones_like(rstd), torch.full_like(rstd, 2.0 ** -17), "rstd / fp64 rstd")
    assert L.dvt_vit_ln_cast_stats(x.data_ptr(), xb.data_ptr(), st.data_ptr(), rows, 1540, C.c_float(eps), _s()) == BADARG


@pytest.mark.parametrize("dim", [1536, 1280])
def test_layernorm_1536_vs_fp64(L, dim):
    """dvt_vit_layernorm on the four row kinds: every element within the bf16 store's 2^-8 of the fp64 LayerNorm, plus what
    an fp32 (mean, rstd) at the bounds above moves it by (2^-17 relative on (x - mean) rstd, the mean's error times rstd)."""
    rows, eps = 300, 1e-6
    g = torch.Generator(device=DEV).manual_seed(dim)
    x = stat_rows(rows, dim, g)
    w, b = torch.randn(dim, generator=g, device=DEV), torch.randn(dim, generator=g, device=DEV)
    y, band, _ = banded16(rows * dim, 2048)
    assert L.dvt_vit_layernorm(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), rows, dim, C.c_float(eps), _s()) == 0
    torch.cuda.synchronize()
    assert_band(band, SENT16, "band")
    x64 = x.double()
    mean, var = x64.mean(1, keepdim=True), x64.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    z = (x64 - mean) * rstd
    ref = z * w.double() + b.double()
    dz = 2.0 ** -16 * z.abs() + 2.0 ** -18 * x64.abs().mean(1, keepdim=True) * rstd + 2.0 ** -22 * x64.abs() * rstd
    assert_close(y.view(rows, dim), ref, 2.0 ** -8 * ref.abs() + 2 * dz * w.double().abs() + 1e-30, "layernorm")
    assert L.dvt_vit_layernorm(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), rows, 1540, C.c_float(eps), _s()) == BADARG


# ------------------------------------------------------------------------------------------ 3. the forward, giant geometry
def _metrics(got, want):
    d = want.shape[-1]
    cos = F.cosine_similarity(got.double().reshape(-1, d), want.double().reshape(-1, d), dim=-1)
    return float(cos.min()), float((got.double() - want.double()).norm() / want.double().norm())


def hold(got, want, cos_bar, err_bar, what, comparator):
    """The project's bar, or -- where it does not hold -- twice the error of `comparator()`, a CPU forward of the same
    arithmetic class (tests/vitg_reference.py) against the same float64 reference: the factor of two covers another
    summation order; the code under test is never its own yardstick.  Prints every figure."""
    cmin, err = _metrics(got, want)
    print(f"{what} vs float64 reference: cos min {cmin:.8f} rel-L2 {err:.3e}")
    if cmin > cos_bar and err <= err_bar:
        return
    ccmp, ecmp = _metrics(comparator(), want)
    print(f"  bar (cos > {cos_bar}, rel-L2 <= {err_bar}) missed; CPU comparator of the same arithmetic class: cos min "
          f"{ccmp:.8f} rel-L2 {ecmp:.3e}")
    assert err <= 2 * ecmp and (1 - cmin) <= 2 * (1 - ccmp), f"{what}: beyond twice the comparator's error"


@pytest.mark.parametrize("n_reg,img,stride", [(0, 518, 14), (4, 518, 14), (4, 112, 7)])
def test_vitg_four_blocks_vs_reference(L, n_reg, img, stride):
    """4 blocks of the ViT-g/14 geometry (dim 1536, 24 heads, SwiGLU 4096), 3 views, against the float64 reference: bf16 and
    exact-fp32 extractors, the cls output, and bit-for-bit independence of max_batch.
    MEASURED (one run, one MI355X): bf16 patch tokens rel-L2 2.86e-2 / 2.64e-2 / 3.07e-2 (the three cases in order), cls rows
    3.09e-2 / 3.06e-2 / 3.53e-2; fp32 6.9e-6 .. 8.9e-6.  The 3e-2 bar is missed by the cls rows and by the 112-px map, and
    `hold` then allows twice the CPU bf16-class comparator's error (2.97e-2 .. 3.51e-2): the EFFECTIVE bf16 bar of this test
    is about 6e-2 .. 7e-2 in rel-L2, not 3e-2."""
    from dvt_amd._lib import DvtError
    from dvt_amd.vit import HipViT, random_state_dict
    sd = random_state_dict(1536, 4, 14, (0 if n_reg else 1) + 37 * 37, seed=40 + n_reg, well_conditioned=True, n_reg=n_reg,
                           mlp="swiglu")
    x = torch.randn(3, 3, img, img, generator=torch.Generator().manual_seed(6))
    want, want_cls = vref.forward_features(sd, x, 14, stride, return_cls=True)
    vit = HipViT(sd, 14, stride, (img, img), DEV)
    assert vit.mlp == "swiglu" and vit.cfg.mlp_dim == 4096 and vit.cfg.heads == 24 and vit.cfg.mlp_kind == 1
    got, cls = vit.forward_features(x.to(DEV), return_cls=True)
    tag = f"ViT-g geometry, 4 blocks, reg {n_reg}, {img}px stride {stride}:"
    cache = {}

    def cmp16(i):  # the bf16 arithmetic class on the CPU: (patch tokens, cls), computed once if a bar is missed
        if "v" not in cache:
            cache["v"] = vref.forward_features(sd, x, 14, stride, return_cls=True, dtype=torch.float32, round_bf16=True)
        return cache["v"][i]

    def cmp32(i):
        if "w" not in cache:
            cache["w"] = vref.forward_features(sd, x, 14, stride, return_cls=True, dtype=torch.float32)
        return cache["w"][i]

    assert got.shape == want.shape
    hold(got.cpu(), want, 0.999, 3e-2, f"{tag} bf16 patch tokens", lambda: cmp16(0))
    hold(cls.cpu(), want_cls, 0.999, 3e-2, f"{tag} bf16 cls", lambda: cmp16(1))
    one = vit.forward_features(x.to(DEV), max_batch=1)
    two = vit.forward_features(x.to(DEV), max_batch=2)
    assert torch.equal(one, got) and torch.equal(two, got), "the result depends on max_batch"
    mid = vit.forward_features(x[:1].to(DEV), n_blocks=2).cpu()
    hold(mid, vref.forward_features(sd, x[:1], 14, stride, n_blocks=2), 0.999, 3e-2, f"{tag} bf16, 2 blocks",
         lambda: vref.forward_features(sd, x[:1], 14, stride, n_blocks=2, dtype=torch.float32, round_bf16=True))
    v32 = HipViT(sd, 14, stride, (img, img), DEV, dtype="float32")
    got32, cls32 = v32.forward_features(x.to(DEV), return_cls=True)
    hold(got32.cpu(), want, 0.999999, 1e-5, f"{tag} fp32 patch tokens", lambda: cmp32(0))
    hold(cls32.cpu(), want_cls, 0.999999, 1e-5, f"{tag} fp32 cls", lambda: cmp32(1))
    assert torch.equal(v32.forward_features(x.to(DEV), max_batch=1), got32)
    with pytest.raises(DvtError, match=r"vit_giant_patch14.*matmul=\"high\""):
        HipViT(sd, 14, stride, (img, img), DEV, dtype="float32", matmul="high")


def test_vitg_full_depth(L):
    """The DINOv2 ViT-g/14 geometry at FULL depth (40 blocks, dim 1536, 24 heads, SwiGLU 4096, 518 x 518, 1 view) through
    PretrainedViTWrapper.get_intermediate_layers, well-conditioned random weights, against the float64 reference.  Bars: the
    project's own from test_vit_large_full_depth (observed there at 24 blocks).  Where one does not hold at 40 blocks the
    test computes a CPU comparator of the same arithmetic class against the same float64 reference (fp32: torch fp32; bf16:
    every matrix operand and stored activation rounded to bf16) and holds the extractor to TWICE the comparator's error.
    MEASURED (one run, one MI355X; also in profiles/vitg/README.md): both bars hold at 40 blocks -- bf16 extractor per-token
    cosine min 0.99962434, rel-L2 2.390e-02; fp32 extractor cosine min 1.00000000, rel-L2 6.049e-06 -- so the comparator was
    not needed here.  The inner layer (index 1, bf16): cosine min 0.99973185, rel-L2 1.523e-02."""
    from dvt_amd.models import PretrainedViTWrapper
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = PretrainedViTWrapper("vit_giant_patch14_dinov2.lvd142m", stride=14, allow_random_init=True)
    assert (w.n_output_dims, w.num_blocks, w.last_layer_index) == (1536, 40, 39)
    sd = w._state_dict
    x = torch.randn(1, 3, 518, 518, generator=torch.Generator().manual_seed(5))
    want = vref.forward_features(sd, x, 14, 14)
    assert want.shape == (1, 37, 37, 1536) and bool(torch.isfinite(want).all())

    got = w.get_intermediate_layers(x.to(DEV), n=[39], reshape=True)[0].permute(0, 2, 3, 1).cpu()
    hold(got, want, 0.999, 3e-2, "ViT-g/14 FULL depth (40 blocks) bf16 extractor",
         lambda: vref.forward_features(sd, x, 14, 14, dtype=torch.float32, round_bf16=True))
    got32 = w.features_nhwc(x.to(DEV), dtype="float32").cpu()
    hold(got32, want, 0.999999, 1e-5, "ViT-g/14 FULL depth (40 blocks) fp32 extractor",
         lambda: vref.forward_features(sd, x, 14, 14, dtype=torch.float32))
    # any layer index, any stride: an inner layer of the same wrapper, and the stride override on a smaller image
    inner = w.get_intermediate_layers(x.to(DEV), n=[1], reshape=False)[0]
    assert inner.shape == (1, 37 * 37, 1536)
    hold(inner.reshape(1, 37, 37, 1536).cpu(), vref.forward_features(sd, x, 14, 14, n_blocks=2), 0.999, 3e-2,
         "ViT-g/14 layer index 1, bf16", lambda: vref.forward_features(sd, x, 14, 14, n_blocks=2, dtype=torch.float32,
                                                                       round_bf16=True))


# ---------------------------------------------------------------------------------------------- 4. the existing models
def test_vitb_two_blocks_bits_equal_the_parent(L):
    """Lifting the width limit did not change the <= 1024 instantiations: a 2-block ViT-B/14 forward (518 x 518, 2 views,
    bf16 and fp32, with and without registers) gives the bits recorded from the parent commit on an MI355X
    (tests/golden/vitb_2block_parent.json: sha256 of the output bytes; tools/record_vit_golden.py wrote it)."""
    import hashlib

    from dvt_amd.vit import HipViT, random_state_dict
    with open(GOLDEN) as f:
        want = json.load(f)["sha256"]
    for n_reg in (0, 4):
        sd = random_state_dict(768, 2, 14, (0 if n_reg else 1) + 37 * 37, seed=9, well_conditioned=True, n_reg=n_reg)
        x = torch.randn(2, 3, 518, 518, generator=torch.Generator().manual_seed(12)).to(DEV)
        for dtype in ("bfloat16", "float32"):
            feat, cls = HipViT(sd, 14, 14, (518, 518), DEV, dtype=dtype).forward_features(x, return_cls=True)
            h = hashlib.sha256(feat.cpu().numpy().tobytes() + cls.cpu().numpy().tobytes()).hexdigest()
            assert h == want[f"{dtype}_reg{n_reg}"], f"ViT-B/14 2 blocks {dtype} reg {n_reg}: bits differ from the parent commit"
