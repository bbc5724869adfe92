"""The XCD-column tile order and the epilogue cache policies of the 256 x 256 bf16 GEMM (csrc/dvt_vit_gemm.hip, dvt_tile_map.h)
change WHERE and WHEN a tile runs and how its stores are cached, never a value: every output of every epilogue is compared
bit for bit with the grouped order (xcols = 1) under the default policy, and the NaN-filled slack behind each output buffer
must stay as it was (a tile mapped twice or outside M x N would show in one of the two).

Shapes: M = 2304 (9 panels: does not divide by the 4 or 2 row sets, some XCDs idle a slot) and M = 256 (one panel: most row
sets are empty); N, K of ViT-B, and N = 1536 with K = 256 (6 N tiles: a request of 4 column sets runs with 2).
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
Q_PRESCALE = 0.125 * 1.4426950408889634
NAN16 = 0x7FC0
NAN32 = 0x7FC00000
XCOLS_AUTO, POLICY_NONE, POLICY_DEFAULT = -70, -200000, -200000 - 128
# (xcols, policy mask): both column orders without any policy, then every policy bit alone, the write-through forms of the two
# that have one (residual stores 2 | 64, hid 8 | 32), every nt bit, the shipped mask (47) and everything at once -- under 2
# column sets where the launch has them
POLICIES = [1, 2, 4, 8, 16, 2 | 64, 8 | 32, 31, 47, 127]
VARIANTS = [(2, 0), (4, 0)] + [(2, p) for p in POLICIES]


def _s():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def L(built_lib):
    import dvt_amd.vit  # noqa: F401 registers signatures
    return built_lib


class order:
    """Context manager: xcols column sets and the policy mask for the block; the defaults restored whatever happens."""

    def __init__(self, L, xcols, policy):
        self.L, self.xcols, self.policy = L, xcols, policy

    def __enter__(self):
        assert self.L.dvt_tune_set(1, -70 - self.xcols) == 0
        assert self.L.dvt_tune_set(1, -200000 - self.policy) == 0

    def __exit__(self, *exc):
        assert self.L.dvt_tune_set(1, XCOLS_AUTO) == 0
        assert self.L.dvt_tune_set(1, POLICY_DEFAULT) == 0


def poisoned(n, slack, dtype):
    """Buffer of n + slack elements, all NaN: (the n outputs, the whole buffer as raw integers)."""
    if dtype == torch.bfloat16:
        raw = torch.full((n + slack,), NAN16, device=DEV, dtype=torch.int16)
    else:
        raw = torch.full((n + slack,), NAN32, device=DEV, dtype=torch.int32)
    return raw[:n].view(dtype), raw


def check_variants(L, run, what, variants=None):
    """run() -> list of (name, raw buffer, n outputs).  Reference: xcols = 1, policy 0; the library's own defaults (auto column
    sets, the shipped mask) are one more variant."""
    with order(L, 1, 0):
        ref = [(name, raw.clone(), n) for name, raw, n in run()]
    for name, raw, n in ref:
        pat = NAN16 if raw.dtype == torch.int16 else NAN32
        assert bool((raw[n:] == pat).all()), f"{what}: reference run wrote behind {name}"
        assert not bool((raw[:n] == pat).all()), f"{what}: reference run wrote nothing to {name}"
    for xcols, policy in (VARIANTS if variants is None else variants) + [(None, None)]:
        if xcols is None:
            got = run()
        else:
            with order(L, xcols, policy):
                got = run()
        for (name, raw, n), (_, want, _) in zip(got, ref):
            assert torch.equal(raw, want), (f"{what}: {name} differs from the default order (or its slack was written) "
                                            f"with xcols {xcols}, policy {policy}")


def rand_bf16(*shape, gen, scale=1.0):
    return (torch.randn(*shape, generator=gen, device=DEV) * scale).bfloat16()


def fold_stats(xf):
    x64 = xf.double()
    return torch.stack([x64.mean(1), 1.0 / torch.sqrt(x64.var(1, unbiased=False) + 1e-6)], 1).float().contiguous()


@pytest.mark.parametrize("s_pad,batch", [(1152, 2), (256, 1)])
def test_qkv_with_vt_bit_identical(L, s_pad, batch):
    """EPI_QKV with the folded LayerNorm, the q pre-scale and V^T (9 N tiles: every request of column sets runs with one)."""
    dim, heads = 768, 12
    m = batch * s_pad
    assert m % 256 == 0
    g = torch.Generator(device=DEV).manual_seed(s_pad + batch)
    xf = torch.randn(m, dim, generator=g, device=DEV) * 2 + torch.randn(m, 1, generator=g, device=DEV)
    x, st = xf.bfloat16(), fold_stats(xf)
    w = rand_bf16(3 * dim, dim, gen=g, scale=2.0 / dim ** 0.5)
    b = torch.randn(3 * dim, generator=g, device=DEV) * 0.3
    cs = w.float().sum(1).contiguous()
    img = heads * 64 * s_pad

    def run():
        qk, qk_raw = poisoned(m * 2 * dim, 256 * 2 * dim, torch.bfloat16)
        vt, vt_raw = poisoned(batch * img, img, torch.bfloat16)
        assert L.dvt_vit_gemm_qkv(x.data_ptr(), w.data_ptr(), b.data_ptr(), qk.data_ptr(), vt.data_ptr(), m, dim, heads, s_pad,
                                  batch, st.data_ptr(), cs.data_ptr(), Q_PRESCALE, _s()) == 0
        torch.cuda.synchronize()
        return [("qk", qk_raw, m * 2 * dim), ("vt", vt_raw, batch * img)]

    check_variants(L, run, f"qkv m {m}")


@pytest.mark.parametrize("m", [2304, 256])
@pytest.mark.parametrize("n,k", [(3072, 768), (1536, 256)])
def test_gelu_lnfold_bit_identical(L, m, n, k):
    """EPI_GELU with the folded LayerNorm (fc1): 12 N tiles (2 and 4 column sets) / 6 (2, and 4 -> 2)."""
    g = torch.Generator(device=DEV).manual_seed(m + n + k)
    xf = torch.randn(m, k, generator=g, device=DEV) * 2 + torch.randn(m, 1, generator=g, device=DEV)
    x, st = xf.bfloat16(), fold_stats(xf)
    w = rand_bf16(n, k, gen=g, scale=2.0 / k ** 0.5)
    b = torch.randn(n, generator=g, device=DEV) * 0.5
    cs = w.float().sum(1).contiguous()

    def run():
        y, y_raw = poisoned(m * n, 256 * n, torch.bfloat16)
        assert L.dvt_vit_gemm_lnfold(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), m, n, k, st.data_ptr(),
                                     cs.data_ptr(), 1, _s()) == 0
        torch.cuda.synchronize()
        return [("hid", y_raw, m * n)]

    check_variants(L, run, f"fc1 {m} x {n} x {k}")


@pytest.mark.parametrize("m", [2304, 256])
@pytest.mark.parametrize("n,k", [(768, 768), (768, 3072), (1536, 256)])
def test_residual_with_xb_and_partials_bit_identical(L, m, n, k):
    """EPI_RESID with its LayerNorm producer side (proj, fc2): x, xb, the partial sums and the finalized stats."""
    g = torch.Generator(device=DEV).manual_seed(m + n + k)
    a = rand_bf16(m, k, gen=g)
    w = rand_bf16(n, k, gen=g, scale=1.0 / k ** 0.5)
    b, gm = torch.randn(n, generator=g, device=DEV), torch.randn(n, generator=g, device=DEV)
    x0 = torch.randn(m * n, generator=g, device=DEV)

    def run():
        x, x_raw = poisoned(m * n, 256 * n, torch.float32)
        x.copy_(x0)
        xb, xb_raw = poisoned(m * n, 256 * n, torch.bfloat16)
        st, st_raw = poisoned(m * 2, 512, torch.float32)
        part, part_raw = poisoned((n // 64) * m * 2, 512, torch.float32)
        assert L.dvt_vit_gemm_residual_stats(a.data_ptr(), w.data_ptr(), b.data_ptr(), gm.data_ptr(), x.data_ptr(),
                                             xb.data_ptr(), st.data_ptr(), part.data_ptr(), m, n, k, C.c_float(1e-6), _s()) == 0
        torch.cuda.synchronize()
        return [("x", x_raw, m * n), ("xb", xb_raw, m * n), ("stats", st_raw, m * 2), ("partials", part_raw, (n // 64) * m * 2)]

    check_variants(L, run, f"residual {m} x {n} x {k}")


def test_defaults_at_a_swept_size_bit_identical(L):
    """The library's defaults differ from the grouped order only on the launches they were measured on: the four GEMMs of a
    ViT-B block at >= 256 row panels.  The smallest such launches (M = 65536) of fc1 (2 column sets, write-through stores) and
    proj (M blocks of 2, nt residual stream), defaults against xcols = 1 without a policy."""
    m, dim, hid = 65536, 768, 3072
    g = torch.Generator(device=DEV).manual_seed(m)
    x = rand_bf16(m, dim, gen=g)
    st = torch.stack([torch.zeros(m, device=DEV), torch.ones(m, device=DEV)], 1).contiguous()
    w1 = rand_bf16(hid, dim, gen=g, scale=2.0 / dim ** 0.5)
    b1 = torch.randn(hid, generator=g, device=DEV) * 0.5
    cs = w1.float().sum(1).contiguous()

    def run_fc1():
        y, y_raw = poisoned(m * hid, 256 * hid, torch.bfloat16)
        assert L.dvt_vit_gemm_lnfold(x.data_ptr(), w1.data_ptr(), b1.data_ptr(), y.data_ptr(), m, hid, dim, st.data_ptr(),
                                     cs.data_ptr(), 1, _s()) == 0
        torch.cuda.synchronize()
        return [("hid", y_raw, m * hid)]

    check_variants(L, run_fc1, "fc1 at 256 panels", variants=[])
    w2 = rand_bf16(dim, dim, gen=g, scale=1.0 / dim ** 0.5)
    b2, gm = torch.randn(dim, generator=g, device=DEV), torch.randn(dim, generator=g, device=DEV)
    x0 = torch.randn(m * dim, generator=g, device=DEV)

    def run_proj():
        xr, x_raw = poisoned(m * dim, 256 * dim, torch.float32)
        xr.copy_(x0)
        xb, xb_raw = poisoned(m * dim, 256 * dim, torch.bfloat16)
        s2, st_raw = poisoned(m * 2, 512, torch.float32)
        part, part_raw = poisoned((dim // 64) * m * 2, 512, torch.float32)
        assert L.dvt_vit_gemm_residual_stats(x.data_ptr(), w2.data_ptr(), b2.data_ptr(), gm.data_ptr(), xr.data_ptr(),
                                             xb.data_ptr(), s2.data_ptr(), part.data_ptr(), m, dim, dim, C.c_float(1e-6), _s()) == 0
        torch.cuda.synchronize()
        return [("x", x_raw, m * dim), ("xb", xb_raw, m * dim), ("stats", st_raw, m * 2), ("partials", part_raw, (dim // 64) * m * 2)]

    check_variants(L, run_proj, "proj at 256 panels", variants=[])


def _vit(dim, depth, img):
    from dvt_amd.vit import HipViT, random_state_dict
    g0 = img // 14
    sd = random_state_dict(dim, depth, 14, 1 + g0 * g0, seed=dim + img, well_conditioned=True)
    return HipViT(sd, 14, 14, (img, img), DEV)


def _forward(vit, imgs, n_blocks):
    cfg = vit.cfg
    n = imgs.shape[0] * cfg.grid_h * cfg.grid_w * cfg.dim
    feat, raw = poisoned(n, 4096, torch.float32)
    vit.forward_features(imgs, n_blocks=n_blocks, out=feat.view(imgs.shape[0], cfg.grid_h, cfg.grid_w, cfg.dim))
    torch.cuda.synchronize()
    return [("features", raw, n)]


@pytest.mark.parametrize("batch", [7, 1])
def test_embed_bit_identical(L, batch):
    """EPI_EMBED (patch GEMM + bias + pos_embed, then the final LayerNorm): dvt_vit_forward with no blocks, dim 768 at 224 x 224,
    several row panels at 7 views and the fewest at one."""
    vit = _vit(768, 1, 224)
    imgs = torch.randn(batch, 3, 224, 224, generator=torch.Generator().manual_seed(batch)).to(DEV)
    check_variants(L, lambda: _forward(vit, imgs, 0), f"embed, {batch} views")


@pytest.mark.parametrize("img", [112, 518])
def test_forward_two_blocks_bit_identical(L, img):
    """One forward of 2 blocks, 3 views (s_pad 96 at 112 x 112, 1376 at 518 x 518) against the default order."""
    vit = _vit(768, 2, img)
    assert vit.cfg.s_pad == (96 if img == 112 else 1376)
    imgs = torch.randn(3, 3, img, img, generator=torch.Generator().manual_seed(img)).to(DEV)
    check_variants(L, lambda: _forward(vit, imgs, 2), f"forward {img} x {img}")


def test_policy_masks_without_a_kernel_are_refused(L):
    """Of the residual stream's three bits a mask holds one or all three: the other pairs have no instantiated kernel."""
    for mask in (3, 5, 6, 3 | 32, 6 | 8, 129):
        assert L.dvt_tune_set(1, -200000 - mask) == -1
    assert L.dvt_tune_set(1, -73) == -1
    assert L.dvt_tune_set(1, POLICY_DEFAULT) == 0 and L.dvt_tune_set(1, XCOLS_AUTO) == 0
