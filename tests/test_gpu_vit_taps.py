"""GPU: several layers, prefix tokens and norm=False from ONE extractor forward (dvt_vit_forward*_taps, HipViT.forward_taps,
PretrainedViTWrapper.get_intermediate_layers / forward, Denoiser.forward(return_class_token=True)).

Shapes (random well-conditioned weights, 56 / 64 px inputs: 17 or 50 tokens per image, 32 or 64 rows per image in bf16 / fp32
and 128 in the bf16x3 mode, so every launch also carries pad rows and phantom rows): ViT-S geometry with 4 blocks, the same
with four register tokens, the DeiT-III layout (position table without a cls row, patch 16), stride 7, and dim 1536 with the
SwiGLU MLP and 2 blocks (the 6-slot rows).  The 4-block shapes tap [0, 2, 3] and, for norm=False, [1, 3]; the 2-block shape
has only [0, 1] to tap.  Modes: bfloat16, float32 and matmul="high" (GELU shapes only: the SwiGLU MLP keeps its refusal).

Bars (none comes from what the code under test gives): bit identity wherever two calls run the same launches; for the
un-normed rows against the float64 reference (tests/taps_reference.py, pinned to tests/backbone_reference.py and
tests/vitg_reference.py by tests/test_vit_taps_cpu.py) the rel-L2 bars those files' forward tests use for the same mode --
GELU shapes (tests/test_gpu_backbones.py): bf16 2e-2, fp32 2e-5; the 1536 SwiGLU shape (tests/test_gpu_vitg.py): bf16 3e-2,
fp32 1e-5; matmul="high" (tests/test_gpu_vit.py): 1e-4 -- and, where a bf16 case misses its bar, the rule of
tests/test_gpu_vitg.py: twice the error of a CPU forward of the same arithmetic class.  The LayerNorm check carries the
bound of test_layernorm_1536_vs_fp64.
MEASURED (one run, one MI355X): profiles/taps/README.md lists every case.
"""
import ctypes as C
import warnings

import pytest
import torch

from tests import taps_reference as tref

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN32 = 0x7FC00000  # the bit pattern torch.full(nan) writes

SHAPES = {
    "s14": dict(dim=384, depth=4, patch=14, img=56, stride=14, n_reg=0, mlp="gelu", pos_rows=17),
    "s14-reg4": dict(dim=384, depth=4, patch=14, img=56, stride=14, n_reg=4, mlp="gelu", pos_rows=16),
    "deit3-layout": dict(dim=384, depth=4, patch=16, img=64, stride=16, n_reg=0, mlp="gelu", pos_rows=16),
    "stride7": dict(dim=384, depth=4, patch=14, img=56, stride=7, n_reg=0, mlp="gelu", pos_rows=17),
    "g1536-swiglu": dict(dim=1536, depth=2, patch=14, img=56, stride=14, n_reg=0, mlp="swiglu", pos_rows=17),
}
MODES = {"bfloat16": ("bfloat16", "highest"), "float32": ("float32", "highest"), "high": ("float32", "high")}
CASES = [pytest.param(s, m, id=f"{s}-{m}") for s in SHAPES for m in MODES if not (m == "high" and SHAPES[s]["mlp"] == "swiglu")]
BARS = {("gelu", "bfloat16"): 2e-2, ("gelu", "float32"): 2e-5, ("gelu", "high"): 1e-4,
        ("swiglu", "bfloat16"): 3e-2, ("swiglu", "float32"): 1e-5}
B3, B5 = 3, 5


def taps_of(shape):
    """(the three-tap list of the bit-identity checks, the pair of the norm=False checks)"""
    return ([0, 2, 3], [1, 3]) if SHAPES[shape]["depth"] == 4 else ([0, 1], [0, 1])


def _s():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def L(built_lib):
    import dvt_amd.vit  # noqa: F401 registers signatures
    return built_lib


_cases, _engines = {}, {}


def case(shape):
    """Weights, five images and the float64 rows after every block of the first three images: computed once per shape, shared
    by every test and never modified."""
    if shape not in _cases:
        from dvt_amd.vit import random_state_dict
        s = SHAPES[shape]
        sd = random_state_dict(s["dim"], s["depth"], s["patch"], s["pos_rows"], seed=17 + len(_cases), well_conditioned=True,
                               n_reg=s["n_reg"], mlp=s["mlp"])
        x = torch.randn(B5, 3, s["img"], s["img"], generator=torch.Generator().manual_seed(23))
        rows, geom = tref.residual_rows(sd, x[:B3], s["patch"], s["stride"], list(range(s["depth"])))
        _cases[shape] = dict(sd=sd, x=x, xd=x.to(DEV), rows=rows, geom=geom, cmp16=None)
    return _cases[shape]


def comparator16(shape):
    """The bf16 arithmetic class on the CPU (every matrix operand rounded to bf16), computed once if a bar is missed."""
    c, s = case(shape), SHAPES[shape]
    if c["cmp16"] is None:
        c["cmp16"] = tref.residual_rows(c["sd"], c["x"][:B3], s["patch"], s["stride"], list(range(s["depth"])),
                                        dtype=torch.float32, round_bf16=True)[0]
    return c["cmp16"]


def engine(shape, mode):
    if (shape, mode) not in _engines:
        from dvt_amd.vit import HipViT
        s = SHAPES[shape]
        dtype, matmul = MODES[mode]
        _engines[(shape, mode)] = HipViT(case(shape)["sd"], s["patch"], s["stride"], (s["img"], s["img"]), DEV, dtype=dtype,
                                         matmul=matmul)
    return _engines[(shape, mode)]


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def rel_l2(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())


def all_rows(fmap, prefix):
    """(map [B, gh, gw, dim], prefix [B, n_prefix, dim]) -> the token rows [B, n_prefix + gh * gw, dim] of the reference."""
    return torch.cat([prefix, fmap.reshape(fmap.shape[0], -1, fmap.shape[-1])], dim=1)


# ---------------------------------------------------------------------------------------------------------- 1. bit identity
@pytest.mark.parametrize("shape,mode", CASES)
def test_normed_taps_are_the_plain_forwards(L, shape, mode):
    """norm=True, batch 3: feat[t] is forward_features(n_blocks = block[t] + 1) and prefix[t][:, 0] its return_cls output, bit
    for bit -- the same launches produce the same residual rows and the tap shares the final norm's device function."""
    vit, xd = engine(shape, mode), case(shape)["xd"][:B3]
    taps, _ = taps_of(shape)
    got = vit.forward_taps(xd, taps, norm=True, return_prefix=True)
    assert len(got) == len(taps)
    gh, gw, n_prefix = case(shape)["geom"]
    for (fmap, prefix), b in zip(got, taps):
        want, cls = vit.forward_features(xd, n_blocks=b + 1, return_cls=True)
        assert fmap.shape == (B3, gh, gw, vit.cfg.dim) and prefix.shape == (B3, n_prefix, vit.cfg.dim)
        assert bool(torch.isfinite(fmap).all()) and bool(torch.isfinite(prefix).all())
        assert same(fmap, want), f"block {b}: the tapped map is not the plain forward's"
        assert same(prefix[:, 0], cls), f"block {b}: the tapped cls row is not the plain forward's"
    plain = vit.forward_taps(xd, taps, norm=True)
    assert all(same(p, g[0]) for p, g in zip(plain, got)), "the maps depend on return_prefix"


# ------------------------------------------------------------------------------------------------------------ 2. norm=False
@pytest.mark.parametrize("shape,mode", CASES)
def test_unnormed_rows(L, shape, mode):
    """norm=False: two taps of one call are the single-tap calls' rows bit for bit (in the bf16 path the fc2 epilogue of a
    tapped inner block also writes xb and the row partials: x comes out the same); the rows hold the mode's rel-L2 bar
    against the float64 reference; and a float64 LayerNorm of them is the norm=True tap within the bound of
    test_layernorm_1536_vs_fp64 (2^-8 |ref| + twice what an fp32 (mean, rstd) moves the row by)."""
    vit, c = engine(shape, mode), case(shape)
    xd, sd = c["xd"][:B3], c["sd"]
    _, pair = taps_of(shape)
    got = vit.forward_taps(xd, pair, norm=False, return_prefix=True)
    normed = vit.forward_taps(xd, pair, norm=True, return_prefix=True)
    bar = BARS[(SHAPES[shape]["mlp"], mode)]
    w64, b64, eps = sd["norm.weight"].double(), sd["norm.bias"].double(), 1e-6
    for (fmap, prefix), (nmap, nprefix), b in zip(got, normed, pair):
        (smap, sprefix), = vit.forward_taps(xd, [b], norm=False, return_prefix=True)
        assert same(fmap, smap) and same(prefix, sprefix), f"block {b}: the rows depend on the other taps of the call"
        rows, want = all_rows(fmap, prefix).cpu(), c["rows"][b]
        assert rows.shape == want.shape and bool(torch.isfinite(rows).all())
        err = rel_l2(rows, want)
        print(f"{shape} {mode} block {b}: un-normed rows vs float64 reference rel-L2 {err:.3e} (bar {bar:.0e})")
        if not err < bar:
            assert mode == "bfloat16", f"block {b}: rel-L2 {err:.3e} misses {bar:.0e}"
            ecmp = rel_l2(comparator16(shape)[b], want)
            print(f"  bar missed; CPU comparator of the same arithmetic class: rel-L2 {ecmp:.3e}")
            assert err <= 2 * ecmp, f"block {b}: rel-L2 {err:.3e} beyond twice the comparator's {ecmp:.3e}"
        x64 = rows.double()
        mean, var = x64.mean(-1, keepdim=True), x64.var(-1, unbiased=False, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + eps)
        z = (x64 - mean) * rstd
        ref = z * w64 + b64
        dz = 2.0 ** -16 * z.abs() + 2.0 ** -18 * x64.abs().mean(-1, keepdim=True) * rstd + 2.0 ** -22 * x64.abs() * rstd
        tol = 2.0 ** -8 * ref.abs() + 2 * dz * w64.abs() + 1e-30
        bad = ~((all_rows(nmap, nprefix).cpu().double() - ref).abs() <= tol)
        assert not bool(bad.any()), f"block {b}: {int(bad.sum())} elements of the norm=True tap are not LayerNorm(norm=False rows)"


# ---------------------------------------------------------------------------------------------------------------- 3. layout
@pytest.mark.parametrize("norm", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("shape,mode", CASES)
def test_layout_guards_and_workspace(L, shape, mode, norm):
    """The C entry point itself: every output sits inside a larger NaN-filled buffer and the workspace is NaN bytes with a
    sentinel band behind it.  No guard element changes, nothing is written behind the workspace, no output holds a NaN (pad
    rows and phantom rows never reach an output), and the bits are HipViT.forward_taps' (a zeroed or reused workspace).
    Prefix rows: row j of prefix[t] is token row j of the reference -- cls, then the registers in their order."""
    from dvt_amd.vit import VitTaps
    vit, c = engine(shape, mode), case(shape)
    xd, cfg = c["xd"][:B3], vit.cfg
    taps, _ = taps_of(shape)
    want = vit.forward_taps(xd, taps, norm=norm, return_prefix=True)
    gh, gw, n_prefix = c["geom"]
    n_map, n_pre, band = B3 * gh * gw * cfg.dim, B3 * n_prefix * cfg.dim, 8192
    fbuf = [torch.full((band + n_map + band,), float("nan"), device=DEV) for _ in taps]
    pbuf = [torch.full((band + n_pre + band,), float("nan"), device=DEV) for _ in taps]
    nbytes = vit.workspace_bytes(B3)
    ws = torch.full((nbytes + 65536,), 0xFF, device=DEV, dtype=torch.uint8)  # NaN in every fp32 / bf16 slot
    ws[nbytes:] = 0xA5
    t = VitTaps()
    t.n_taps, t.norm = len(taps), int(norm)
    for i, b in enumerate(taps):
        t.block[i], t.feat[i], t.prefix[i] = b, fbuf[i][band:].data_ptr(), pbuf[i][band:].data_ptr()
    fn = {"bfloat16": L.dvt_vit_forward_taps, "float32": L.dvt_vit_forward_f32_taps, "high": L.dvt_vit_forward_f32x3_taps}[mode]
    assert fn(C.byref(cfg), C.byref(vit.weights), xd.data_ptr(), C.byref(t), B3, ws.data_ptr(), _s()) == 0
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all()), "written behind the workspace"
    for i, b in enumerate(taps):
        for buf, n, what in ((fbuf[i], n_map, "map"), (pbuf[i], n_pre, "prefix")):
            guard = torch.cat([bits(buf[:band]), bits(buf[band + n:])])
            assert bool((guard == NAN32).all()), f"block {b}: a guard element of the {what} output changed"
            assert not bool(torch.isnan(buf[band:band + n]).any()), f"block {b}: the {what} output holds a NaN"
        assert same(fbuf[i][band:band + n_map].view(B3, gh, gw, cfg.dim), want[i][0]), f"block {b}: map bits"
        assert same(pbuf[i][band:band + n_pre].view(B3, n_prefix, cfg.dim), want[i][1]), f"block {b}: prefix bits"
        if not norm:  # the order of the prefix rows: row j is nearer to token row j of the reference forward than to any other
            # prefix row of it (the tokens are distinct random vectors; how near is test_unnormed_rows' business)
            got = want[i][1].cpu()
            for j in range(n_prefix):
                errs = [rel_l2(got[:, j], c["rows"][b][:, k]) for k in range(n_prefix)]
                assert min(range(n_prefix), key=errs.__getitem__) == j, \
                    f"block {b}: prefix row {j} is not token row {j} of the reference ({errs})"
    # a NULL prefix output drops the prefix rows and leaves the map as it is
    t.prefix[0] = None
    pbuf[0].fill_(float("nan"))
    fbuf[0].fill_(float("nan"))
    assert fn(C.byref(cfg), C.byref(vit.weights), xd.data_ptr(), C.byref(t), B3, ws.data_ptr(), _s()) == 0
    torch.cuda.synchronize()
    assert bool((bits(pbuf[0]) == NAN32).all()) and same(fbuf[0][band:band + n_map].view(B3, gh, gw, cfg.dim), want[0][0])


# -------------------------------------------------------------------------------------------------------------- 4. batching
@pytest.mark.parametrize("shape,mode", CASES)
def test_batching_and_preallocated_maps(L, shape, mode):
    """B = 5 in launches of at most 2 views gives the bits of one launch, written into slices of a feature store."""
    vit, xd = engine(shape, mode), case(shape)["xd"]
    taps, _ = taps_of(shape)
    assert len(vit.launch_plan(B5, 2)) >= 3
    one = vit.forward_taps(xd, taps, return_prefix=True, max_batch=128)
    gh, gw, _ = case(shape)["geom"]
    store = torch.full((len(taps), B5, gh, gw, vit.cfg.dim), float("nan"), device=DEV)
    many = vit.forward_taps(xd, taps, return_prefix=True, outs=[store[i] for i in range(len(taps))], max_batch=2)
    for i, ((m1, p1), (m2, p2)) in enumerate(zip(one, many)):
        assert m2.data_ptr() == store[i].data_ptr(), "forward_taps did not write into the map it was given"
        assert same(m1, m2) and same(p1, p2), "the result depends on max_batch"
    from dvt_amd._lib import DvtError
    for bad in ([], [1, 1], [2, 1], [vit.cfg.depth], [-1]):
        with pytest.raises(DvtError):
            vit.forward_taps(xd, bad)
    with pytest.raises(DvtError):
        vit.forward_taps(xd, taps, outs=[store[0]])


# ----------------------------------------------------------------------------------------------- 5. one forward, 6. the API
@pytest.fixture(scope="module")
def wrapper():
    from dvt_amd.models import PretrainedViTWrapper
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = PretrainedViTWrapper("vit_small_patch14_reg4_dinov2.lvd142m", stride=14, img_size=56, allow_random_init=True)
    assert (w.num_blocks, w.n_output_dims) == (12, 384)
    return w


@pytest.fixture(scope="module")
def images():
    return torch.randn(B5, 3, 56, 56, generator=torch.Generator().manual_seed(31)).to(DEV)


def test_get_intermediate_layers_runs_one_forward(L, wrapper, images, monkeypatch):
    """With the library's forwards wrapped by counters and launches capped at 2 views: n=[0, 1, 3] with prefix tokens calls
    the tapped entry once per chunk of the launch plan and the plain forwards not at all."""
    monkeypatch.setenv("DVT_VIT_MAX_VIEWS", "2")
    plan = wrapper._engine(images.device).launch_plan(B5)
    assert len(plan) >= 3 and sum(plan) == B5
    counts = {}

    def counted(name):
        real = getattr(L, name)

        def call(*a):
            counts[name] = counts.get(name, 0) + 1
            return real(*a)
        return call

    names = [f"dvt_vit_forward{a}{k}" for a in ("", "_f32", "_f32x3") for k in ("", "_cls", "_taps")]
    for name in names:
        monkeypatch.setattr(L, name, counted(name))
    out = wrapper.get_intermediate_layers(images, n=[0, 1, 3], return_prefix_tokens=True)
    assert counts == {"dvt_vit_forward_taps": len(plan)}, counts
    assert len(out) == 3 and all(f.shape == (B5, 384, 4, 4) and p.shape == (B5, 5, 384) for f, p in out)


def test_public_api(L, wrapper, images):
    """Shapes and types of every combination of reshape / return_prefix_tokens / norm; the single-index norm=True call the
    drivers make returns the bits of features_nhwc; forward(x) is the final-normed cls token; the Denoiser hands it on."""
    from dvt_amd.models import Denoiser
    x = images[:B3]
    for reshape in (True, False):
        for with_prefix in (True, False):
            for norm in (True, False):
                out = wrapper.get_intermediate_layers(x, n=[3, -1], reshape=reshape, return_prefix_tokens=with_prefix, norm=norm)
                assert isinstance(out, list) and len(out) == 2
                for item, idx in zip(out, (3, 11)):
                    f, p = item if with_prefix else (item, None)
                    assert isinstance(item, tuple) == with_prefix
                    assert f.shape == ((B3, 384, 4, 4) if reshape else (B3, 16, 384)) and f.dtype == torch.float32 and f.is_cuda
                    nhwc = f.permute(0, 2, 3, 1) if reshape else f.reshape(B3, 4, 4, 384)
                    if norm:
                        assert same(nhwc, wrapper.features_nhwc(x, idx)), f"layer {idx}: not the bits of features_nhwc"
                    else:
                        assert not same(nhwc, wrapper.features_nhwc(x, idx))
                    if with_prefix:
                        assert p.shape == (B3, 5, 384) and p.dtype == torch.float32 and p.is_cuda
    for idx in (0, 11):  # stage 1, stage 3, the video demo
        f = wrapper.get_intermediate_layers(x, n=[idx], reshape=True)[-1].permute(0, 2, 3, 1)
        assert same(f, wrapper.features_nhwc(x, idx))
    feats, cls = wrapper.features_nhwc(x, return_cls=True)
    assert same(wrapper.forward(x), cls) and same(wrapper(x), cls) and cls.shape == (B3, 384)
    assert same(feats, wrapper.features_nhwc(x))
    den = Denoiser(4, 4, 384, wrapper, device=DEV, seed=0)
    plain = den.forward(x)
    denoised, tokens = den.forward(x, return_class_token=True)
    assert same(denoised, plain) and same(tokens, cls)
    d = den.forward(x, return_dict=True, return_class_token=True)
    assert same(d["class_tokens"], cls) and same(d["denoised_feats"], plain)
    assert den.forward(x, return_dict=True)["class_tokens"] is None
    raw, raw_tokens = den.forward(x, return_class_token=True, norm=False)
    assert raw.shape == plain.shape and not same(raw_tokens, cls)
