"""Element-level parity of the bf16 extractor's GEMM epilogues (csrc/dvt_vit_epilogue.h, launched by csrc/dvt_vit_gemm.hip) against fp64, one epilogue at a time.

The whole-forward tests (tests/test_gpu_vit.py) hold every token to a cosine of 0.999; that cannot see a structural error in
one epilogue (a V^T chunk stored into the wrong image moves an attention output by almost nothing).  Here every entry point
that runs an epilogue of dvt_vit_forward is compared ELEMENT BY ELEMENT with a reference computed in fp64 from the same
bf16-rounded operands (and the same fp32 (mean, rstd) where the LayerNorm is folded): what remains is fp32 accumulation
(bounded by K * 2^-24 * sum |a| |w|, computed per element) plus the final rounding (2^-8 relative for a bf16 output).

Every output is filled with NaN before the call (an element the kernel should have written and did not fails), and a
sentinel band lies behind every output, sized to hold the whole overrun of the V^T store as it was before GemmBArgs::vt_rows
(the phantom rows of the last 256-row tile: ceil(m / s_pad) - batch images): such a store lands in the test's own memory.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
BADARG = -1
GEMM_DEFAULT = 4  # dvt_tune_set(1, v): 4 = 256x256 8-phase ring (default), 3 = 256x128 ping-pong, 1 = 128x128 (register epilogue)
Q_PRESCALE = 0.125 * 1.4426950408889634  # log2(e) / 8: what dvt_vit_forward's qkv epilogue applies to q
U = 2.0 ** -24  # fp32 unit roundoff
NAN16 = 0x7FC0  # bf16 quiet NaN
SENT16 = 0x5A5A  # bf16 sentinel (a finite value no kernel here produces by chance in a whole band)


def _s():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def L(built_lib):
    import dvt_amd.vit  # noqa: F401 registers signatures
    return built_lib


def gemm_schedule(L, v):
    """Context manager: GEMM schedule v for the block, the default restored whatever happens."""
    class _Sched:
        def __enter__(self):
            assert L.dvt_tune_set(1, v) == 0

        def __exit__(self, *exc):
            assert L.dvt_tune_set(1, GEMM_DEFAULT) == 0
    return _Sched()


def banded16(n, band):
    """bf16 buffer of n NaN elements + `band` sentinel elements behind: (output view, band view as int16, whole buffer)."""
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
    """|got - ref| <= tol element by element (NaN fails); reports the worst element."""
    got = got.double()
    err = (got - ref).abs()
    bad = ~(err <= tol)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements out of tolerance; first at {idx}: "
                             f"got {float(got.flatten()[i])!r} want {float(ref.flatten()[i])!r} tol {float(tol.flatten()[i]):.3g}")


def bf16_tol(ref, acc):
    """Output rounded to bf16 once from an fp32 value whose error is <= acc: 2^-8 |ref| + 2 acc (+ fp32 epilogue rounding)."""
    return 2.0 ** -8 * ref.abs() + 2.0 * acc + 2.0 ** -22 * ref.abs() + 1e-30


def acc_bound(a, w):
    """fp32 accumulation bound of a . w^T over K: K * 2^-24 * (|a| . |w|^T), fp64."""
    return a.shape[1] * U * (a.double().abs() @ w.double().abs().t())


def phantom_images(m, s_pad, batch):
    """V^T images behind image batch - 1 that the phantom rows of an m-row launch map to (row // s_pad): where an unguarded
    V^T store would land."""
    return -(-m // s_pad) - batch


def x3_band_images(m, s_pad, batch):
    """Images of sentinel band behind the bf16x3 attention scratch that hold every unguarded V^T store: V^T lo is the last
    array of the scratch and has one spare image (index batch) of its own, so its stores reach phantom_images - 1 images past
    the end (V^T hi's land inside the scratch, in the V^T lo array)."""
    return max(1, phantom_images(m, s_pad, batch) - 1)


def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def rand_bf16(*shape, gen, scale=1.0, offset=0.0):
    return (torch.randn(*shape, generator=gen, device=DEV) * scale + offset).bfloat16()


# ---------------------------------------------------------------------------------------------------------- 1. qkv epilogue
QKV_CASES = [(32, 1), (96, 1), (64, 2), (160, 5), (1376, 2), (1408, 3), (1376, 1), (32, 3)]  # (s_pad, batch)
QKV_FORMS = [(768, False, 0.0), (768, True, Q_PRESCALE), (128, False, Q_PRESCALE), (128, False, 0.0)]  # (dim, fold, q_scale)


def qkv_operands(m, dim, fold, seed):
    """x bf16 [m, dim], w bf16 [3 dim, dim], b fp32 [3 dim] (+ fp32 stats [m, 2] and column sums [3 dim] for the fold).
    Folded: x = bf16 of a residual stream whose rows have their own offset / scale, w = bf16(gamma (.) W)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = 3 * dim
    w = rand_bf16(n, dim, gen=g, scale=2.0 / dim ** 0.5)
    w[:, :8] += 0.05  # asymmetric columns: a transposed fragment shows
    b = torch.randn(n, generator=g, device=DEV) * 0.3
    if not fold:
        x = rand_bf16(m, dim, gen=g) + torch.linspace(-0.5, 0.5, dim, device=DEV).bfloat16()
        return x.bfloat16(), w, b, None, None
    xf = torch.randn(m, dim, generator=g, device=DEV) * (0.5 + torch.rand(m, 1, generator=g, device=DEV) * 3)
    xf += torch.randn(m, 1, generator=g, device=DEV) * 4  # per-row offsets: the mean * cs term matters
    x = xf.bfloat16()
    x64 = xf.double()
    mean = x64.mean(1)
    rstd = 1.0 / torch.sqrt(x64.var(1, unbiased=False) + 1e-6)
    stats = torch.stack([mean, rstd], 1).float().contiguous()
    cs = w.float().sum(1).contiguous()
    return x, w, b, stats, cs


def qkv_reference(x, w, b, stats, cs, q_scale, dim):
    """fp64 (value, accumulation bound) of the qkv epilogue's fp32 value for every row and column."""
    acc = x.double() @ w.double().t()
    bound = acc_bound(x, w)
    if stats is None:
        v = acc + b.double()
    else:
        mu, rs = stats[:, 0:1].double(), stats[:, 1:2].double()
        v = rs * (acc - mu * cs.double()) + b.double()
        # the fp32 correction: rstd * (acc - mean * cs) + b' after an fp32 acc
        bound = rs * (bound + 4 * U * (acc.abs() + (mu * cs.double()).abs())) + 2 * U * v.abs()
    if q_scale != 0.0:
        v[:, :dim] *= q_scale
        bound[:, :dim] *= q_scale
    return v, bound


@pytest.mark.parametrize("variant", [1, 3, 4])
@pytest.mark.parametrize("dim,fold,q_scale", QKV_FORMS)
@pytest.mark.parametrize("s_pad,batch", QKV_CASES)
def test_qkv_epilogue_vs_fp64(L, s_pad, batch, dim, fold, q_scale, variant):
    """dvt_vit_gemm_qkv: q | k into qk [m, 2 dim] and V^T per head into vt [batch, heads, 64, s_pad], every element, pad
    tokens included (attention reads them with P = 0, so they must be finite); the phantom rows behind batch * s_pad get
    q | k and NO V^T -- the band behind vt (room for every image the phantom rows would map to) stays untouched."""
    heads = dim // 64
    m = (batch * s_pad + 255) // 256 * 256
    real = batch * s_pad
    x, w, b, stats, cs = qkv_operands(m, dim, fold, seed=s_pad * 31 + batch * 7 + dim)
    img = heads * 64 * s_pad
    over = max(1, phantom_images(m, s_pad, batch))  # images the phantom rows' V^T reached before vt_rows
    qk, qk_band, _ = banded16(m * 2 * dim, 128 * 2 * dim)
    vt, vt_band, _ = banded16(batch * img, over * img)
    with gemm_schedule(L, variant):
        rc = L.dvt_vit_gemm_qkv(x.data_ptr(), w.data_ptr(), b.data_ptr(), qk.data_ptr(), vt.data_ptr(), m, dim, heads,
                                s_pad, batch, stats.data_ptr() if fold else None, cs.data_ptr() if fold else None,
                                q_scale, _s())
        torch.cuda.synchronize()
    if fold and variant == 1:
        # the 128 x 128 kernel's register epilogue has no folded form: refused, nothing written
        assert rc == BADARG
        assert bool(qk.isnan().all()) and bool(vt.isnan().all())
        return
    assert rc == 0
    assert_band(vt_band, SENT16, f"vt band (s_pad {s_pad}, batch {batch})")
    assert_band(qk_band, SENT16, "qk band")
    v, bound = qkv_reference(x, w, b, stats, cs, q_scale, dim)
    assert_close(qk.view(m, 2 * dim), v[:, :2 * dim], bf16_tol(v[:, :2 * dim], bound[:, :2 * dim]), "q | k")
    vref = v[:real, 2 * dim:].reshape(batch, s_pad, heads, 64).permute(0, 2, 3, 1)
    vb = bound[:real, 2 * dim:].reshape(batch, s_pad, heads, 64).permute(0, 2, 3, 1)
    assert_close(vt.view(batch, heads, 64, s_pad), vref, bf16_tol(vref, vb), "V^T")


def test_qkv_rejects_bad_arguments(L):
    dim, heads, s_pad, batch = 768, 12, 96, 1
    m = 256
    x = torch.zeros(m, dim, device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(3 * dim, dim, device=DEV, dtype=torch.bfloat16)
    b = torch.zeros(3 * dim, device=DEV)
    qk = torch.zeros(m + 128, 2 * dim, device=DEV, dtype=torch.bfloat16)
    vt = torch.zeros(batch + 1, heads, 64, s_pad, device=DEV, dtype=torch.bfloat16)
    st = torch.zeros(m, 2, device=DEV)
    call = lambda m_, s_pad_, st_, cs_, dim_=dim: L.dvt_vit_gemm_qkv(  # noqa: E731
        x.data_ptr(), w.data_ptr(), b.data_ptr(), qk.data_ptr(), vt.data_ptr(), m_, dim_, dim_ // 64, s_pad_, batch, st_, cs_,
        0.0, _s())
    assert call(128, s_pad, None, None) == BADARG  # m is not batch * s_pad rounded up to 256
    assert call(512, s_pad, None, None) == BADARG
    assert call(m, 80, None, None) == BADARG  # s_pad % 32
    assert call(m, s_pad, st.data_ptr(), None) == BADARG  # stats without column sums
    assert call(m, s_pad, st.data_ptr(), b.data_ptr(), dim_=128) == BADARG  # folded: 3 dim % 256
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- 2. fc1 with the fold
@pytest.mark.parametrize("variant", [1, 3, 4])
@pytest.mark.parametrize("fold,gelu", [(True, 1), (False, 1), (False, 0)])
@pytest.mark.parametrize("m,n,k", [(512, 3072, 768), (768, 1024, 256)])
def test_fc1_lnfold_vs_fp64(L, m, n, k, fold, gelu, variant):
    """dvt_vit_gemm_lnfold: GELU_erf(rstd (x_b . W'^T - mean cs) + b') per element against fp64 (the erf approximation adds
    <= 1e-6 absolute), and the unfolded GELU / bias forms.  The folded form on the 128 x 128 schedule is refused."""
    g = torch.Generator(device=DEV).manual_seed(m + n + k + 10 * fold + gelu)
    w = rand_bf16(n, k, gen=g, scale=2.0 / k ** 0.5)
    b = torch.randn(n, generator=g, device=DEV) * 0.5
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
    if gelu:
        v = gelu64(v)
        bound = 1.13 * bound + 1e-6  # |GELU'| <= 1.13; the A-S 7.1.28 erfc in fp32
    y, band, _ = banded16(m * n, 4096)
    with gemm_schedule(L, variant):
        rc = L.dvt_vit_gemm_lnfold(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), m, n, k,
                                   st.data_ptr() if fold else None, cs.data_ptr() if fold else None, gelu, _s())
        torch.cuda.synchronize()
    if fold and variant == 1:
        assert rc == BADARG and bool(y.isnan().all())
        return
    assert rc == 0
    assert_band(band, SENT16, "fc1 band")
    assert_close(y.view(m, n), v, bf16_tol(v, bound), f"fc1 fold={fold} gelu={gelu}")


# -------------------------------------------------------------------------------------------------- 3. fold statistics
def stat_rows(rows, dim, gen):
    """fp32 rows of four kinds: N(0, 1); a large common offset (mean 1e3, std 1: a one-pass variance cancels); tiny spread
    (mean -5, std 0.01); wide (std 100)."""
    x = torch.randn(rows, dim, generator=gen, device=DEV)
    kind = torch.arange(rows, device=DEV) % 4
    x[kind == 1] = x[kind == 1] + 1e3
    x[kind == 2] = x[kind == 2] * 0.01 - 5
    x[kind == 3] = x[kind == 3] * 100
    return x.contiguous()


def stats64(x, eps):
    x64 = x.double()
    mean = x64.mean(1)
    var = x64.var(1, unbiased=False)
    return mean, var, 1.0 / torch.sqrt(var + eps)


@pytest.mark.parametrize("rows,dim", [(301, 768), (256, 128), (97, 1024), (4352, 768)])
def test_ln_cast_stats_vs_fp64(L, rows, dim):
    """dvt_vit_ln_cast_stats: xb = bf16(x) bit for bit, (mean, rstd) two-pass to fp32 precision -- also on rows with a large
    common offset, where a one-pass E[x^2] - mean^2 would lose every digit."""
    eps = 1e-6
    x = stat_rows(rows, dim, torch.Generator(device=DEV).manual_seed(rows + dim))
    xb, xb_band, _ = banded16(rows * dim, 2048)
    st, st_band, _ = banded32(rows * 2, 256)
    assert L.dvt_vit_ln_cast_stats(x.data_ptr(), xb.data_ptr(), st.data_ptr(), rows, dim, C.c_float(eps), _s()) == 0
    torch.cuda.synchronize()
    assert_band(xb_band, SENT16, "xb band")
    assert_band(st_band, 0x5A5A5A5A, "stats band")
    assert torch.equal(xb.view(rows, dim).view(torch.int16), x.bfloat16().view(torch.int16)), "xb is not bf16(x)"
    mean, var, rstd = stats64(x, eps)
    st = st.view(rows, 2).double()
    assert_close(st[:, 0], mean, 2.0 ** -18 * x.double().abs().mean(1), "mean")
    assert_close(st[:, 1] / rstd, torch.ones_like(rstd), torch.full_like(rstd, 2.0 ** -17), "rstd / fp64 rstd")


@pytest.mark.parametrize("variant", [1, 3, 4])
@pytest.mark.parametrize("m,n,k", [(512, 768, 768), (768, 1024, 256)])
def test_gemm_residual_stats_vs_fp64(L, m, n, k, variant):
    """dvt_vit_gemm_residual_stats: x += gamma (a . w^T + b) as in test_gemm_residual_vs_torch, xb = bf16(new x) bit for bit,
    and the (mean, rstd) of the new x rows from the per-block partial sums.  That variance is ONE pass in fp32 (E[x^2] -
    mean^2, documented in include/dvt_vit.h): its error bound is 2^-16 (mean^2 + var), tight for centred rows, vacuous for
    rows with a large common offset (checked for finiteness there).  Schedules other than the 256 x 256 one are refused."""
    eps = 1e-6
    g = torch.Generator(device=DEV).manual_seed(m + n + k)
    a = rand_bf16(m, k, gen=g)
    w = rand_bf16(n, k, gen=g, scale=1.0 / k ** 0.5)
    b, gm = torch.randn(n, generator=g, device=DEV), torch.randn(n, generator=g, device=DEV)
    x0 = stat_rows(m, n, g)
    x, x_band, _ = banded32(m * n, 1024)
    x.copy_(x0.flatten())
    xb, xb_band, _ = banded16(m * n, 2048)
    st, st_band, _ = banded32(m * 2, 256)
    part, part_band, _ = banded32((n // 64) * m * 2, 256)
    with gemm_schedule(L, variant):
        rc = L.dvt_vit_gemm_residual_stats(a.data_ptr(), w.data_ptr(), b.data_ptr(), gm.data_ptr(), x.data_ptr(),
                                           xb.data_ptr(), st.data_ptr(), part.data_ptr(), m, n, k, C.c_float(eps), _s())
        torch.cuda.synchronize()
    if variant != 4:
        assert rc == BADARG
        assert torch.equal(x.view(m, n), x0) and bool(xb.isnan().all()) and bool(st.isnan().all())
        return
    assert rc == 0
    for band, pat, what in ((x_band, 0x5A5A5A5A, "x"), (xb_band, SENT16, "xb"), (st_band, 0x5A5A5A5A, "stats"),
                            (part_band, 0x5A5A5A5A, "partials")):
        assert_band(band, pat, what + " band")
    v = a.double() @ w.double().t() + b.double()
    want = x0.double() + gm.double() * v
    tol = gm.double().abs() * (acc_bound(a, w) + 3 * U * v.abs()) + 2 * U * want.abs() + 1e-30
    xg = x.view(m, n)
    assert_close(xg, want, tol, "x")
    assert torch.equal(xb.view(m, n).view(torch.int16), xg.bfloat16().view(torch.int16)), "xb is not bf16(new x)"
    mean, var, rstd = stats64(xg, eps)  # of the x the kernel wrote
    st = st.view(m, 2).double()
    assert bool(torch.isfinite(st).all())
    assert_close(st[:, 0], mean, 2.0 ** -18 * xg.double().abs().mean(1), "mean")
    var_got = 1.0 / st[:, 1] ** 2 - eps
    assert_close(var_got, var, 2.0 ** -16 * (mean ** 2 + var) + 2.0 ** -20 * var + 2 * eps, "variance")
    centred = mean ** 2 <= var
    assert int(centred.sum()) >= m // 2
    assert_close(st[centred, 1] / rstd[centred], torch.ones_like(rstd[centred]),
                 torch.full_like(rstd[centred], 2.0 ** -14), "rstd / fp64 rstd (centred rows)")


# ----------------------------------------------------------------------------------- 4. patch embedding + final LayerNorm
EMBED_CASES = [  # (img_h, img_w, patch, stride, n_reg, batch): the im2col branch each one takes
    (518, 518, 14, 14, 0, 1),  # im2col_pairs_kernel<14>
    (224, 224, 16, 16, 0, 3),  # im2col_pairs_kernel<16>
    (56, 56, 14, 7, 0, 3),     # generic (odd stride)
    (98, 97, 14, 14, 0, 1),    # generic (odd width), rectangular grid 7 x 6
    (56, 98, 14, 14, 0, 3),    # pairs<14>, rectangular grid 4 x 7: swapped grid_h / grid_w would show
    (70, 84, 14, 14, 4, 3),    # register tokens: n_prefix 5, pos_has_cls 0
]


def build_vit(dim, depth, patch, stride, img_h, img_w, n_reg, seed):
    from dvt_amd.vit import HipViT, random_state_dict
    g0 = max(img_h, img_w) // patch
    sd = random_state_dict(dim, depth, patch, (0 if n_reg else 1) + g0 * g0, seed=seed, well_conditioned=True, n_reg=n_reg)
    return sd, HipViT(sd, patch, stride, (img_h, img_w), DEV)


@pytest.mark.parametrize("img_h,img_w,patch,stride,n_reg,batch", EMBED_CASES)
def test_patch_embedding_and_final_norm_vs_fp64(L, img_h, img_w, patch, stride, n_reg, batch):
    """dvt_vit_forward with n_blocks = 0: im2col (bf16 image) -> patch GEMM -> EPI_EMBED (+ bias + pos_embed of the right
    row) -> final LayerNorm -> the NHWC patch tokens, per element against fp64 of the bf16 image and bf16 patch_w."""
    from dvt_amd.vit import resample_pos_embed
    dim = 128
    sd, vit = build_vit(dim, 1, patch, stride, img_h, img_w, n_reg, seed=img_h + img_w + n_reg)
    cfg = vit.cfg
    gh, gw = cfg.grid_h, cfg.grid_w
    assert (cfg.n_prefix, cfg.pos_has_cls) == ((5, 0) if n_reg else (1, 1))
    img = torch.randn(batch, 3, img_h, img_w, generator=torch.Generator().manual_seed(batch)).to(DEV)
    n_out = batch * gh * gw * dim
    feat, band, _ = banded32(n_out, 4096)
    vit.forward_features(img, n_blocks=0, out=feat.view(batch, gh, gw, dim))
    torch.cuda.synchronize()
    assert_band(band, 0x5A5A5A5A, "feature band")
    # fp64 reference
    W = sd["patch_embed.proj.weight"].reshape(dim, -1).bfloat16().double().to(DEV)
    cols = F.unfold(img.bfloat16().double(), kernel_size=patch, stride=stride)  # [B, 3 p^2, gh * gw], row-major tokens
    assert cols.shape[-1] == gh * gw
    cols = cols.transpose(1, 2)
    acc = cols @ W.t()
    bound = cols.shape[-1] * U * (cols.abs() @ W.abs().t())
    pos = resample_pos_embed(sd["pos_embed"], (gh, gw), cfg.pos_has_cls).reshape(-1, dim).double().to(DEV)
    pos = pos[cfg.pos_has_cls:]  # the patch rows
    x = acc + sd["patch_embed.proj.bias"].double().to(DEV) + pos
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + cfg.ln_eps)
    nw, nb = sd["norm.weight"].double().to(DEV), sd["norm.bias"].double().to(DEV)
    y = xc * rstd * nw + nb
    tol = nw.abs() * rstd * (2 * bound + 16 * U * x.abs().amax(-1, keepdim=True)) + 2.0 ** -18 * (y.abs() + nb.abs()) + 1e-6
    assert_close(feat.view(batch, gh * gw, dim), y, tol, "patch tokens after the final LayerNorm")


# ------------------------------------------------------------------------------- 5. workspace contract of the forward
# (56 x 56, 7 views: the last image's query block reads rows of qk behind the 256-row tiles, which nothing writes)
WS_CASES = [(128, 56, 1), (128, 56, 3), (128, 56, 7), (128, 112, 1), (128, 518, 1), (128, 518, 2),
            (768, 56, 1), (768, 56, 3), (768, 112, 1), (768, 518, 1), (768, 518, 3)]  # (dim, img, batch)


@pytest.mark.parametrize("dim,img,batch", WS_CASES)
def test_forward_workspace_contract(L, dim, img, batch):
    """dvt_vit_forward (bf16, depth 2; LayerNorm folded at dim 768, LayerNorm kernels at dim 128): the result does not depend
    on the workspace's contents -- zero-filled, NaN bytes, or left over from a launch of more views (HipViT._workspace
    reuses one for every smaller launch) give the same features bit for bit -- and nothing is written behind
    dvt_vit_workspace_bytes or behind the feature rows."""
    from dvt_amd import _lib
    _, vit = build_vit(dim, 2, 14, 14, img, img, 0, seed=dim + img)
    cfg = vit.cfg
    lib = _lib.lib()
    big = batch + 2
    ws_bytes = int(lib.dvt_vit_workspace_bytes(C.byref(cfg), batch))
    big_bytes = int(lib.dvt_vit_workspace_bytes(C.byref(cfg), big))
    assert 0 < ws_bytes < big_bytes
    imgs = torch.randn(big, 3, img, img, generator=torch.Generator().manual_seed(img + batch)).to(DEV)
    n_feat = cfg.grid_h * cfg.grid_w * dim
    WBAND = 1 << 16

    def run(ws, n_views, images):
        feat, fband, _ = banded32(n_views * n_feat, 4096)
        assert lib.dvt_vit_forward(C.byref(cfg), C.byref(vit.weights), images.data_ptr(), feat.data_ptr(), n_views, 2,
                                   ws.data_ptr(), _s()) == 0
        torch.cuda.synchronize()
        assert_band(fband, 0x5A5A5A5A, "feature band")
        return feat.clone()

    def workspace(nbytes, fill):
        buf = torch.full((nbytes + WBAND,), fill, device=DEV, dtype=torch.uint8)
        buf[nbytes:] = 0xA5
        return buf

    ws0 = workspace(ws_bytes, 0)
    ref = run(ws0, batch, imgs)
    assert bool(torch.isfinite(ref).all())
    wsn = workspace(ws_bytes, 0xFF)  # NaN in every fp32 / bf16 slot
    got_nan = run(wsn, batch, imgs)
    wsb = workspace(big_bytes, 0)
    run(wsb, big, imgs.flip(0).contiguous())  # another launch of more views first
    got_reuse = run(wsb, batch, imgs)
    for ws, nbytes, what in ((ws0, ws_bytes, "zeroed"), (wsn, ws_bytes, "NaN-filled"), (wsb, big_bytes, "reused")):
        assert bool((ws[nbytes:] == 0xA5).all()), f"{what} workspace: written behind dvt_vit_workspace_bytes"
    assert torch.equal(got_nan.view(torch.int32), ref.view(torch.int32)), "a NaN-filled workspace changed the features"
    assert torch.equal(got_reuse.view(torch.int32), ref.view(torch.int32)), "a reused workspace changed the features"


# ----------------------------------------------------------------------------- 6. split epilogues of the `high` mode
def check_split(hi, lo, ref, bound, what):
    """(hi, lo) = (bf16(v), bf16(v - hi)) of the kernel's fp32 v: |lo| within half an ulp of hi, hi + lo = v to 2^-16."""
    h, l_ = hi.double(), lo.double()
    assert bool((l_.abs() <= 2.0 ** -8 * h.abs()).all()), f"{what}: lo is not the remainder of a rounded hi"
    assert_close(h + l_, ref, 2.0 ** -16 * ref.abs() + 2 * bound + 1e-30, what + " hi + lo")
    assert_close(hi, ref, bf16_tol(ref, bound), what + " hi")


@pytest.mark.parametrize("dim", [768, 128])
@pytest.mark.parametrize("s_pad,batch", [(128, 1), (128, 2), (1408, 3), (1408, 2)])
def test_qkv_x3_split_epilogue_vs_fp64(L, s_pad, batch, dim):
    """dvt_vit_gemm_qkv_x3: q | k (hi, lo) [m, 2 dim] and V^T (hi, lo) [batch, heads, 64, s_pad] in the attention scratch,
    against fp64; the spare V^T image of each part (index `batch`) and a band behind the scratch stay untouched."""
    heads = dim // 64
    m = (batch * s_pad + 255) // 256 * 256
    real = batch * s_pad
    k = 3 * dim  # the [hi | hi | lo] operand width of the fp32 mode
    g = torch.Generator(device=DEV).manual_seed(s_pad + batch + dim)
    a = rand_bf16(m, k, gen=g)
    w = rand_bf16(3 * dim, k, gen=g, scale=1.0 / k ** 0.5)
    b = torch.randn(3 * dim, generator=g, device=DEV) * 0.3
    nbytes = int(L.dvt_vit_attention_x3_scratch_bytes(batch, heads, s_pad))
    n16 = nbytes // 2
    img = heads * 64 * s_pad
    assert n16 == 4 * m * dim + 2 * (batch + 1) * img
    sc, band, _ = banded16(n16, x3_band_images(m, s_pad, batch) * img)
    assert L.dvt_vit_gemm_qkv_x3(a.data_ptr(), w.data_ptr(), b.data_ptr(), sc.data_ptr(), m, dim, heads, s_pad, batch, k,
                                 _s()) == 0
    torch.cuda.synchronize()
    assert_band(band, SENT16, "x3 scratch band")
    v = a.double() @ w.double().t() + b.double()
    bound = acc_bound(a, w) + 2 * U * v.abs()
    ql = m * 2 * dim
    vh = 2 * ql
    vl = vh + (batch + 1) * img
    check_split(sc[:ql].view(m, 2 * dim), sc[ql:vh].view(m, 2 * dim), v[:, :2 * dim], bound[:, :2 * dim], "q | k")
    vref = v[:real, 2 * dim:].reshape(batch, s_pad, heads, 64).permute(0, 2, 3, 1)
    vb = bound[:real, 2 * dim:].reshape(batch, s_pad, heads, 64).permute(0, 2, 3, 1)
    check_split(sc[vh:vh + batch * img].view(batch, heads, 64, s_pad), sc[vl:vl + batch * img].view(batch, heads, 64, s_pad),
                vref, vb, "V^T")
    raw = sc.view(torch.int16)
    for start, what in ((vh + batch * img, "V^T hi"), (vl + batch * img, "V^T lo")):
        assert bool((raw[start:start + img] == NAN16).all()), f"{what}: the spare image `batch` was written"


def test_qkv_x3_rejects_unaligned_rows(L):
    """s_pad % 128 != 0 is refused before anything is written (its one consumer, the presplit attention, needs it).  Were the
    check missing, the phantom rows 32..255 would store V^T into images 1..7: the band holds all 6 that lie past the scratch."""
    dim, heads, s_pad, batch = 128, 2, 32, 1
    m, k = 256, 3 * dim
    nbytes = int(L.dvt_vit_attention_x3_scratch_bytes(batch, heads, s_pad))
    assert x3_band_images(m, s_pad, batch) == 6
    sc, band, _ = banded16(nbytes // 2, x3_band_images(m, s_pad, batch) * heads * 64 * s_pad)
    a = torch.zeros(m, k, device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(3 * dim, k, device=DEV, dtype=torch.bfloat16)
    b = torch.zeros(3 * dim, device=DEV)
    assert L.dvt_vit_gemm_qkv_x3(a.data_ptr(), w.data_ptr(), b.data_ptr(), sc.data_ptr(), m, dim, heads, s_pad, batch, k,
                                 _s()) == BADARG
    torch.cuda.synchronize()
    assert bool((sc.view(torch.int16) == NAN16).all())
    assert_band(band, SENT16, "x3 scratch band")


@pytest.mark.parametrize("m,n,k", [(512, 3072, 2304), (256, 512, 384)])
def test_gelu_x3_split_epilogue_vs_fp64(L, m, n, k):
    """dvt_vit_gemm_gelu_x3: out3 [m, 3 n] = [hi | hi | lo] of GELU(a . w^T + b), the next GEMM's A row."""
    g = torch.Generator(device=DEV).manual_seed(m + n + k)
    a = rand_bf16(m, k, gen=g)
    w = rand_bf16(n, k, gen=g, scale=2.0 / k ** 0.5)
    b = torch.randn(n, generator=g, device=DEV) * 0.5
    out, band, _ = banded16(m * 3 * n, 4096)
    assert L.dvt_vit_gemm_gelu_x3(a.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k, _s()) == 0
    torch.cuda.synchronize()
    assert_band(band, SENT16, "out3 band")
    pre = a.double() @ w.double().t() + b.double()
    v = gelu64(pre)
    bound = 1.13 * (acc_bound(a, w) + 2 * U * pre.abs()) + 1e-6
    o = out.view(m, 3, n)
    assert torch.equal(o[:, 0].view(torch.int16), o[:, 1].view(torch.int16)), "the two hi copies differ"
    check_split(o[:, 0], o[:, 2], v, bound, "GELU split")
