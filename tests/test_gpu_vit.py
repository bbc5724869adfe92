"""GPU parity of the HIP ViT extractor against the fp32 oracle (oracle/vit.py).

Tolerance: the HIP path computes with bf16 operands / fp32 accumulation (the reference's
`--dtype bfloat16` mode), the oracle in fp32: single kernels agree to bf16 rounding
(rel 1e-2 of the tensor scale), whole forwards to per-token cosine >= 0.999 with
well-conditioned random weights (LayerScale O(1), so every block term is exercised).
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from oracle import vit as ovit

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATTN_DEFAULT = 2   # dvt_tune_set(1, -500 - v): attention kernel of the bf16 extractor (1: round 2 [lab builds], 2: round 3)
ATTN_MASK_DEFAULT = 15  # dvt_tune_set(1, -510 - mask): schedule mask of the round-3 kernel (csrc/dvt_vit_attn.hip, attention_kernel_v2)
# (kernel, mask).  The product library contains the shipped pair only; tests/test_gpu_lab.py runs the same checks on the
# developer build's other kernels / masks (round 2; round 3 as first measured; the two-barrier ping-pong experiment)
# "log2q" (round 6): the kernel dvt_vit_forward launches -- dvt_vit_attention_log2q, q PRE-SCALED by log2(e) / 8 (the qkv GEMM's
# epilogue does that on its fp32 accumulators), logits in units of log2, the S chain started from -max; the same checks
ATTN_CASES = [(2, 15), "log2q"]
# ("log2q", x): developer builds of the log2-domain kernel, schedule-mask bits x toggled (dvt_tune_set(1, -540 - x)): the other P.V
# order, no group pattern for the K reads, the ablation builds (idle waves compute / whole tail tile), P packed behind the V^T reads
LAB_ATTN_CASES = [(1, 0), (2, 0), (2, 79), ("log2q", 2), ("log2q", 514), ("log2q", 384), ("log2q", 1024), ("log2q", 16384), ("log2q", 32768), ("log2q", 32768 + 65536)]
Q_PRESCALE = 0.125 * 1.4426950408889634


def attn_q(q, attn_variant):
    """(the bf16 q the kernel is handed, the q of the reference's logits q . k) for one attention entry point."""
    if attn_variant == "log2q" or attn_variant[0] == "log2q":
        qp = (q.float() * Q_PRESCALE).bfloat16()
        return qp, qp.double() * 0.6931471805599453  # 2^(q' . k) = e^(ln 2 q' . k)
    qb = q.bfloat16()
    return qb, qb.double() * 0.125


def run_attention(L, attn_variant, qk, vt, out, batch, heads, s_pad, n_valid):
    if attn_variant == "log2q":
        return L.dvt_vit_attention_log2q(qk.data_ptr(), vt.data_ptr(), out.data_ptr(), batch, heads, s_pad, n_valid, _s())
    if attn_variant[0] == "log2q":
        assert L.dvt_tune_set(1, -540 - attn_variant[1]) == 0
        try:
            return L.dvt_vit_attention_log2q(qk.data_ptr(), vt.data_ptr(), out.data_ptr(), batch, heads, s_pad, n_valid, _s())
        finally:
            assert L.dvt_tune_set(1, -540) == 0
    set_attn(L, *attn_variant)
    try:
        return L.dvt_vit_attention(qk.data_ptr(), vt.data_ptr(), out.data_ptr(), batch, heads, s_pad, n_valid, _s())
    finally:
        set_attn(L)


def set_attn(L, variant=ATTN_DEFAULT, mask=ATTN_MASK_DEFAULT):
    assert L.dvt_tune_set(1, -500 - variant) == 0 and L.dvt_tune_set(1, -510 - mask) == 0
GEMM_DEFAULT = 4   # dvt_tune_set(1, v): ViT GEMM schedule (product: 4 = 256x256 8-phase ring, 3 = 256x128 ping-pong, 1 = 128x128)


def _s():
    return torch.cuda.current_stream().cuda_stream


_KEEP = []


def P(t):
    """Device pointer with the device copy kept alive (no data_ptr() of temporaries)."""
    t = t.detach().to(DEV).contiguous()
    _KEEP.append(t)
    return t.data_ptr()


def rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-30))


@pytest.fixture(scope="module")
def L(built_lib):
    import dvt_amd.vit  # noqa: F401 registers signatures
    return built_lib


@pytest.mark.parametrize("m,n,k", [(128, 128, 64), (256, 384, 192), (384, 768, 768), (128, 2304, 768),
                                   (1408, 768, 3072), (256, 128, 640), (512, 256, 128), (2816, 768, 768)])
def test_gemm_bias_vs_torch(L, m, n, k):
    torch.manual_seed(m + n + k)
    # asymmetric operands: catches transposed / permuted fragment layouts
    x = (torch.randn(m, k) + torch.linspace(-1, 1, k)[None, :] * torch.linspace(0.5, 2, m)[:, None]).bfloat16()
    w = (torch.randn(n, k) / k ** 0.5 + torch.linspace(-0.02, 0.03, n)[:, None]).bfloat16()
    b = torch.randn(n)
    want = x.float() @ w.float().t() + b
    y = torch.empty((m, n), device=DEV, dtype=torch.bfloat16)
    assert L.dvt_vit_gemm_bias(P(x), P(w), P(b),
                               y.data_ptr(), m, n, k, _s()) == 0
    assert rel(y.float(), want) < 6e-3, (m, n, k)


RESID_SHAPES = [(512, 256, 128), (2816, 768, 768), (1408, 768, 3072), (256, 384, 192), (1792, 768, 768)]


@pytest.mark.parametrize("variant", [1, 3, 4])
@pytest.mark.parametrize("m,n,k", RESID_SHAPES)
def test_gemm_residual_vs_torch(L, m, n, k, variant):
    check_gemm_residual_vs_torch(L, m, n, k, variant)


def check_gemm_residual_vs_torch(L, m, n, k, variant):
    """x += gamma * (a @ w^T + b) (LayerScale + residual epilogue) on every GEMM schedule: 4 = 256x256 8-phase
    ring, 3 = 256x128 ping-pong, 1 = 128x128 (lab builds: 0 = 256x256 two-stage, 5 / 10 = re-schedules of 4).
    Every element is checked: the epilogue once lost single dwords of a 16-byte store to a VGPR-overwrite hazard."""
    torch.manual_seed(m + n + k)
    a = torch.randn(m, k).bfloat16()
    w = (torch.randn(n, k) / k ** 0.5).bfloat16()
    b, gm, x0 = torch.randn(n), torch.randn(n), torch.randn(m, n)
    want = x0 + gm * (a.float() @ w.float().t() + b)
    x = x0.to(DEV).contiguous()
    assert L.dvt_tune_set(1, variant) == 0
    try:
        assert L.dvt_vit_gemm_residual(P(a), P(w), P(b), P(gm), x.data_ptr(), m, n, k, _s()) == 0
        torch.cuda.synchronize()
    finally:
        L.dvt_tune_set(1, GEMM_DEFAULT)
    err = (x.cpu() - want).abs()
    assert float(err.max()) < 2e-3 * float(want.abs().max()), (variant, (m, n, k), float(err.max()))


@pytest.mark.parametrize("variant", [1, 3, 4])
def test_gemm_bias_variants(L, variant):
    check_gemm_bias_variants(L, variant)


def check_gemm_bias_variants(L, variant):
    """the GEMM schedules against torch on the four ViT-B shapes (one M panel pair each); lab builds: 6 / 7 = the 4-wave
    persistent kernel (csrc/lab/dvt_vit_gemm4w.inc; flush per tile / deferred epilogue) where K >= 640, else 8p"""
    for n, k in [(2304, 768), (768, 768), (3072, 768), (768, 3072), (768, 640)]:
        torch.manual_seed(n + k)
        m = 512
        x = torch.randn(m, k).bfloat16()
        w = (torch.randn(n, k) / k ** 0.5).bfloat16()
        b = torch.randn(n)
        want = x.float() @ w.float().t() + b
        y = torch.empty((m, n), device=DEV, dtype=torch.bfloat16)
        assert L.dvt_tune_set(1, variant) == 0
        try:
            assert L.dvt_vit_gemm_bias(P(x), P(w), P(b), y.data_ptr(), m, n, k, _s()) == 0
            torch.cuda.synchronize()
        finally:
            L.dvt_tune_set(1, GEMM_DEFAULT)
        assert rel(y.float(), want) < 6e-3, (variant, n, k)


@pytest.mark.parametrize("dim,depth,img,stride,n_reg", [(128, 2, 56, 7, 0), (128, 2, 56, 14, 4),
                                                        (256, 2, 98, 7, 4), (384, 1, 70, 14, 0)])
def test_vit_strides_and_register_tokens_vs_oracle(L, dim, depth, img, stride, n_reg):
    """the stride override (vit_wrapper.py:78-91; overlapping patches + pos_embed resampled
    from the checkpoint's grid) and the *_reg4_* models (4 register tokens between cls and the patches,
    pos_embed on the patches only, prefix tokens stripped from the returned map); ViT-S width."""
    from dvt_amd.vit import HipViT, random_state_dict
    g0 = img // 14                       # the checkpoint's grid (stride = patch)
    g = (img - 14) // stride + 1         # the grid actually produced
    sd = random_state_dict(dim, depth, 14, (0 if n_reg else 1) + g0 * g0, seed=dim + stride,
                           well_conditioned=True, n_reg=n_reg)
    x = torch.randn(3, 3, img, img, generator=torch.Generator().manual_seed(2))
    want = ovit.forward_features(sd, x, 14, stride)
    vit = HipViT(sd, 14, stride, (img, img), DEV)
    assert (vit.cfg.grid_h, vit.cfg.n_prefix, vit.cfg.pos_has_cls) == (g, 1 + n_reg, int(n_reg == 0))
    got = vit.forward_features(x.to(DEV)).cpu()
    assert got.shape == want.shape == (3, g, g, dim)
    cos = F.cosine_similarity(got.reshape(-1, dim), want.reshape(-1, dim), dim=-1)
    err = float((got - want).norm() / want.norm())
    print(f"ViT dim={dim} stride={stride} reg={n_reg}: cos mean {cos.mean():.6f} min {cos.min():.6f} rel-L2 {err:.4f}")
    assert cos.min() > 0.999 and err < 2e-2


def test_gemm_rejects_unaligned(L):
    assert L.dvt_vit_gemm_bias(1, 1, None, 1, 100, 128, 64, None) == -1
    assert L.dvt_vit_gemm_bias(1, 1, None, 1, 128, 128, 32, None) == -1


@pytest.mark.parametrize("dim", [768, 1024, 128])
def test_layernorm_vs_torch(L, dim):
    torch.manual_seed(dim)
    x = torch.randn(300, dim) * 3 + 1.5
    w, b = torch.randn(dim), torch.randn(dim)
    y = torch.empty((300, dim), device=DEV, dtype=torch.bfloat16)
    assert L.dvt_vit_layernorm(P(x), P(w), P(b),
                               y.data_ptr(), 300, dim, 1e-6, _s()) == 0
    assert rel(y.float(), F.layer_norm(x, (dim,), w, b, 1e-6)) < 5e-3


ATTN_SHAPES = [(2, 2, 128, 100), (1, 3, 256, 256), (1, 2, 1408, 1370), (1, 1, 128, 1), (1, 1, 256, 65)]


@pytest.mark.parametrize("attn_variant", ATTN_CASES)
@pytest.mark.parametrize("batch,heads,s_pad,n_valid", ATTN_SHAPES)
def test_attention_vs_torch(L, batch, heads, s_pad, n_valid, attn_variant):
    check_attention_vs_torch(L, batch, heads, s_pad, n_valid, attn_variant)


def check_attention_vs_torch(L, batch, heads, s_pad, n_valid, attn_variant):
    torch.manual_seed(s_pad + heads)
    dim = heads * 64
    q = torch.randn(batch, s_pad, heads, 64)
    k = torch.randn(batch, s_pad, heads, 64) + torch.linspace(-1, 1, 64)  # asymmetric
    v = torch.randn(batch, s_pad, heads, 64) * torch.linspace(0.5, 1.5, 64)
    kb, vb = k.bfloat16(), v.bfloat16()
    qb, qref = attn_q(q, attn_variant)
    att = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", qref, kb.double()[:, :n_valid]), -1)
    want = torch.einsum("bhqk,bkhd->bqhd", att, vb.double()[:, :n_valid]).reshape(batch, s_pad, dim).float()
    qk = torch.cat([qb.reshape(batch * s_pad, dim), kb.reshape(batch * s_pad, dim)], 1).contiguous().to(DEV)
    vt = vb.permute(0, 2, 3, 1).contiguous().to(DEV)  # [batch, heads, 64, s_pad]
    out = torch.empty((batch * s_pad, dim), device=DEV, dtype=torch.bfloat16)
    assert run_attention(L, attn_variant, qk, vt, out, batch, heads, s_pad, n_valid) == 0
    torch.cuda.synchronize()
    got = out.float().reshape(batch, s_pad, dim).cpu()
    assert rel(got[:, :n_valid], want[:, :n_valid]) < 2e-2
    assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize("attn_variant", ATTN_CASES)
@pytest.mark.parametrize("batch,heads,s_pad,n_valid", [(3, 2, 1376, 1370), (2, 1, 160, 150), (1, 2, 1376, 1376), (2, 2, 32, 20),
                                                       (2, 1, 1376, 1345), (2, 1, 96, 65), (1, 2, 1312, 1300)])
def test_attention_row_pitch_not_a_multiple_of_128(L, batch, heads, s_pad, n_valid, attn_variant):
    """Round 6: an image owns s_pad rows with s_pad a multiple of 32 only (1370 tokens -> 1376 instead of 1408).  The kernel
    still walks blocks of 128 queries and tiles of 64 keys: the last block / tile of an image hangs over into the NEXT image's
    rows (read, masked / not stored) -- every image's valid rows must come out right (nobody else's block stores into them),
    the pad rows of the output are written by nobody else either, and what lies behind the last image (the 128 rows of qk the
    caller keeps allocated; anything behind vt) may hold ANY bit pattern: NaN here -- a reused workspace re-carved for another
    batch does hold such patterns, and 0 x NaN once poisoned whole images (round 6, first cut: V^T was read behind its rows)."""
    torch.manual_seed(s_pad + heads + batch)
    dim = heads * 64
    q = torch.randn(batch, s_pad, heads, 64)
    k = torch.randn(batch, s_pad, heads, 64) + torch.linspace(-1, 1, 64)
    v = torch.randn(batch, s_pad, heads, 64) * torch.linspace(0.5, 1.5, 64)
    kb, vb = k.bfloat16(), v.bfloat16()
    qb, qref = attn_q(q, attn_variant)
    att = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", qref, kb.double()[:, :n_valid]), -1)
    want = torch.einsum("bhqk,bkhd->bqhd", att, vb.double()[:, :n_valid]).reshape(batch, s_pad, dim).float()
    rows = batch * s_pad
    qk = torch.full((rows + 128, 2 * dim), float("nan"), dtype=torch.bfloat16)  # slack: NaN
    qk[:rows] = torch.cat([qb.reshape(rows, dim), kb.reshape(rows, dim)], 1)
    vt = torch.full((batch + 1, heads, 64, s_pad), float("nan"), dtype=torch.bfloat16)
    vt[:batch] = vb.permute(0, 2, 3, 1)
    qk, vt = qk.to(DEV), vt.to(DEV)
    out = torch.full((rows + 128, dim), 7.0, device=DEV, dtype=torch.bfloat16)
    assert run_attention(L, attn_variant, qk, vt, out, batch, heads, s_pad, n_valid) == 0
    torch.cuda.synchronize()
    assert bool((out[rows:].float() == 7.0).all()), "a query block past the last image stored its rows"
    got = out[:rows].float().reshape(batch, s_pad, dim).cpu()
    assert bool(torch.isfinite(got).all())
    for b in range(batch):
        assert rel(got[b, :n_valid], want[b, :n_valid]) < 2e-2, b
    assert run_attention(L, attn_variant, qk, vt, out, batch, heads, s_pad + 8, n_valid) == -1


SPIKES = [(0, 1.5), (1, 1.5), (5, 1.5), (20, 1.5), (21, 1.5), (7, 1.0), (13, 1.15)]


@pytest.mark.parametrize("attn_variant", ATTN_CASES)
@pytest.mark.parametrize("spike_tile,gain", SPIKES)
def test_attention_late_max_growth(L, attn_variant, spike_tile, gain):
    check_attention_late_max_growth(L, attn_variant, spike_tile, gain)


def check_attention_late_max_growth(L, attn_variant, spike_tile, gain):
    """Online softmax with a running max that JUMPS late (programming guide 5.4 rule 26): one key row of tile
    `spike_tile` is aligned with a few queries so that its logit exceeds everything seen before by far more than the
    deferred-max threshold of the v2 kernel (8), forcing the rescale of o / l in the middle of the key loop -- a branch
    bounded random data takes only on the first tile.  Full-tensor fp64 reference; every query row is checked."""
    torch.manual_seed(spike_tile)
    batch, heads, s_pad, n_valid = 1, 2, 1408, 1370
    dim = heads * 64
    q = torch.randn(batch, s_pad, heads, 64)
    k = torch.randn(batch, s_pad, heads, 64)
    v = torch.randn(batch, s_pad, heads, 64)
    key = 64 * spike_tile + 17
    k[:, key] = 0.0
    for qi in (3, 200, 777, 1369):       # queries in different waves / workgroups
        k[:, key] += q[:, qi] * gain      # q . k ~ gain |q|^2 ~ 96 -> logit ~ 12 after the 1/8 scale at gain 1.5, others ~ N(0, 1);
                                          # gains 1.0 / 1.15 put it AT the deferred-max threshold (8): some rows above, some below
    kb, vb = k.bfloat16(), v.bfloat16()
    qb, qref = attn_q(q, attn_variant)
    att = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", qref, kb.double()[:, :n_valid]), -1)
    want = torch.einsum("bhqk,bkhd->bqhd", att, vb.double()[:, :n_valid]).reshape(batch, s_pad, dim)
    assert float(att[..., key].max()) > (0.5 if gain >= 1.5 else 0.2)  # the spiked key really dominates some rows
    qk = torch.cat([qb.reshape(batch * s_pad, dim), kb.reshape(batch * s_pad, dim)], 1).contiguous().to(DEV)
    vt = vb.permute(0, 2, 3, 1).contiguous().to(DEV)
    out = torch.empty((batch * s_pad, dim), device=DEV, dtype=torch.bfloat16)
    assert run_attention(L, attn_variant, qk, vt, out, batch, heads, s_pad, n_valid) == 0
    torch.cuda.synchronize()
    got = out.double().reshape(batch, s_pad, dim).cpu()
    err = (got[:, :n_valid] - want[:, :n_valid]).abs().amax(dim=-1)  # per query row
    assert float(err.max()) < 3e-2, (attn_variant, spike_tile, int(err.argmax()), float(err.max()))
    assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize("dim,depth,img,batch,n_blocks", [(128, 2, 56, 3, None), (256, 3, 98, 2, 2),
                                                          (768, 2, 518, 2, None)])
def test_vit_forward_vs_oracle(L, dim, depth, img, batch, n_blocks):
    from dvt_amd.vit import HipViT, random_state_dict
    g = (img - 14) // 14 + 1
    sd = random_state_dict(dim, depth, 14, 1 + g * g, seed=dim, well_conditioned=True)
    x = torch.randn(batch, 3, img, img, generator=torch.Generator().manual_seed(1))
    want = ovit.forward_features(sd, x, 14, 14, n_blocks=n_blocks)
    vit = HipViT(sd, 14, 14, (img, img), DEV)
    got = vit.forward_features(x.to(DEV), n_blocks=n_blocks).cpu()
    assert got.shape == want.shape == (batch, g, g, dim)
    cos = F.cosine_similarity(got.reshape(-1, dim), want.reshape(-1, dim), dim=-1)
    err = float((got - want).norm() / want.norm())
    print(f"ViT dim={dim} depth={depth} img={img}: cos mean {cos.mean():.6f} min {cos.min():.6f} rel-L2 {err:.4f}")
    assert cos.min() > 0.999 and err < 2e-2
    # batching must not change results (workspace reuse, pad rows)
    got2 = vit.forward_features(x.to(DEV), n_blocks=n_blocks, max_batch=1).cpu()
    assert torch.equal(got, got2)
    # round 6: q as it is + the round-3..5 attention kernel (dvt_tune_set(1, -530)) instead of q * log2(e) / 8 + the log2-domain
    # kernel (default): another bf16 rounding of q, the same error class against the oracle
    assert L.dvt_tune_set(1, -530) == 0
    try:
        got3 = vit.forward_features(x.to(DEV), n_blocks=n_blocks).cpu()
    finally:
        assert L.dvt_tune_set(1, -531) == 0
    cos3 = F.cosine_similarity(got3.reshape(-1, dim), want.reshape(-1, dim), dim=-1)
    err3 = float((got3 - want).norm() / want.norm())
    print(f"   ... with q unscaled (-530): cos mean {cos3.mean():.6f} min {cos3.min():.6f} rel-L2 {err3:.4f}; "
          f"between the two: {float((got3 - got).norm() / got.norm()):.4f}")
    assert cos3.min() > 0.999 and err3 < 2e-2 and not torch.equal(got3, got)


def test_wrapper_api_full_depth(L):
    """PretrainedViTWrapper drop-in surface with the real ViT-B/14 geometry (random weights)."""
    import warnings

    from dvt_amd.models import MODEL_LIST, PretrainedViTWrapper
    assert len(MODEL_LIST) == 20
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vit = PretrainedViTWrapper("vit_base_patch14_dinov2.lvd142m", stride=14,
                                   allow_random_init=True).to(DEV).eval()
    assert (vit.n_output_dims, vit.num_blocks, vit.last_layer_index, vit.patch_size) == (768, 12, 11, 14)
    norm = vit.transformation.transforms[-1]
    assert len(norm.mean) == 3 and len(norm.std) == 3
    x = torch.randn(1, 3, 518, 518, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        out = vit.get_intermediate_layers(x.to(DEV), n=[11], reshape=True)
    assert isinstance(out, list) and out[-1].shape == (1, 768, 37, 37)
    nhwc = out[-1].permute(0, 2, 3, 1)
    want = ovit.forward_features(vit._state_dict, x, 14, 14)
    cos = F.cosine_similarity(nhwc.reshape(-1, 768).cpu(), want.reshape(-1, 768), dim=-1)
    print(f"ViT-B/14 full depth vs oracle: cos mean {cos.mean():.6f} min {cos.min():.6f}")
    assert cos.min() > 0.999  # observed 0.9996 (profiles/r03/final/gpu_suite.txt)
    with pytest.raises(NotImplementedError):
        PretrainedViTWrapper("vit_base_patch16_224.mae", stride=16)


@pytest.mark.parametrize("batch,heads,s_pad,n_valid", [(2, 2, 128, 100), (1, 3, 256, 256), (1, 2, 1408, 1370), (3, 2, 1376, 1370),
                                                        (2, 1, 160, 150), (2, 2, 32, 20)])
def test_attention_f32_vs_torch(L, batch, heads, s_pad, n_valid):
    """fp32 attention of the `--dtype float32` extractor (exact-fp32 MFMA, P kept in the accumulator registers)"""
    torch.manual_seed(s_pad + heads)
    dim = heads * 64
    q = torch.randn(batch, s_pad, heads, 64)
    k = torch.randn(batch, s_pad, heads, 64) + torch.linspace(-1, 1, 64)  # asymmetric
    v = torch.randn(batch, s_pad, heads, 64) * torch.linspace(0.5, 1.5, 64)
    att = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q.double() * 0.125, k.double()[:, :n_valid]), -1)
    want = torch.einsum("bhqk,bkhd->bqhd", att, v.double()[:, :n_valid]).reshape(batch, s_pad, dim)
    rows = batch * s_pad
    qkv = torch.full((rows + 128, 3 * dim), float("nan"))  # what the last block reads behind the last image: NaN, never stored
    qkv[:rows] = torch.cat([q.reshape(rows, dim), k.reshape(rows, dim), v.reshape(rows, dim)], 1)
    qkv = qkv.to(DEV)
    out = torch.full((rows + 128, dim), 7.0, device=DEV, dtype=torch.float32)
    assert L.dvt_vit_attention_f32(qkv.data_ptr(), out.data_ptr(), batch, heads, s_pad, n_valid, _s()) == 0
    torch.cuda.synchronize()
    assert bool((out[rows:] == 7.0).all()), "a query block behind the last image stored its rows"
    got = out[:rows].reshape(batch, s_pad, dim).cpu()
    assert rel(got[:, :n_valid], want[:, :n_valid]) < 2e-5
    assert bool(torch.isfinite(got).all())
    assert L.dvt_vit_attention_f32(qkv.data_ptr(), out.data_ptr(), batch, heads, s_pad + 8, n_valid, _s()) == -1


@pytest.mark.parametrize("dim,depth,img,stride,n_reg", [(128, 2, 56, 14, 0), (256, 2, 98, 7, 4), (768, 2, 518, 14, 0)])
def test_vit_forward_f32_vs_oracle(L, dim, depth, img, stride, n_reg):
    """`--dtype float32` (the reference default: autocast off): fp32 operands everywhere.  Against the fp32
    oracle the result must be fp32-roundoff close, two orders tighter than the bf16 extractor."""
    from dvt_amd.vit import HipViT, random_state_dict
    g0 = img // 14
    sd = random_state_dict(dim, depth, 14, (0 if n_reg else 1) + g0 * g0, seed=dim + 1, well_conditioned=True,
                           n_reg=n_reg)
    x = torch.randn(2, 3, img, img, generator=torch.Generator().manual_seed(3))
    want = ovit.forward_features(sd, x, 14, stride)
    vit32 = HipViT(sd, 14, stride, (img, img), DEV, dtype="float32")
    got = vit32.forward_features(x.to(DEV)).cpu()
    assert got.shape == want.shape
    err = float((got - want).norm() / want.norm())
    cos = F.cosine_similarity(got.reshape(-1, dim), want.reshape(-1, dim), dim=-1)
    bf = HipViT(sd, 14, stride, (img, img), DEV).forward_features(x.to(DEV)).cpu()
    err_bf = float((bf - want).norm() / want.norm())
    print(f"fp32 ViT dim={dim} stride={stride} reg={n_reg}: rel-L2 {err:.2e} (bf16 extractor: {err_bf:.2e}), "
          f"cos min {cos.min():.8f}")
    assert err < 2e-5 and cos.min() > 0.999999
    assert err < 0.02 * err_bf


@pytest.mark.parametrize("m,n,k", [(256, 768, 768), (512, 2304, 768), (256, 768, 3072), (128, 384, 640)])
def test_linear_f32x3_vs_fp64(L, m, n, k):
    """The opt-in bf16x3 linear layer (torch's float32 matmul precision "high"; include/dvt_vit.h): operands with a wide
    dynamic range, fp64 reference.  The split is exact to 2^-17 and the product keeps everything but a_lo w_lo, so the
    result must sit ~1e-5 from fp64 -- three orders tighter than a plain bf16 GEMM, two above true fp32."""
    g = torch.Generator().manual_seed(m + n + k)
    x = (torch.randn(m, k, generator=g) * torch.exp(2.0 * torch.randn(m, 1, generator=g))).float()
    w = (torch.randn(n, k, generator=g) / k ** 0.5 * torch.exp(torch.randn(n, 1, generator=g))).float()
    b = torch.randn(n, generator=g)
    want = x.double() @ w.double().T + b.double()
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    x3 = torch.empty(m, 3 * k, device=DEV, dtype=torch.bfloat16)
    w3 = torch.empty(n, 3 * k, device=DEV, dtype=torch.bfloat16)
    y = torch.empty(m, n, device=DEV)
    assert L.dvt_vit_split3(wd.data_ptr(), w3.data_ptr(), n, k, 1, 0, _s()) == 0
    assert L.dvt_vit_linear_f32x3(xd.data_ptr(), w3.data_ptr(), bd.data_ptr(), y.data_ptr(), x3.data_ptr(), m, n, k, _s()) == 0
    torch.cuda.synchronize()
    # the split itself: hi + lo == x to 2^-16 relative, layouts [hi | hi | lo] / [hi | lo | hi]
    xs, ws = x3.float().cpu(), w3.float().cpu()
    assert torch.equal(xs[:, :k], xs[:, k:2 * k]) and torch.equal(ws[:, :k], ws[:, 2 * k:])
    assert torch.equal(xs[:, :k], x.bfloat16().float())
    assert float(((xs[:, :k] + xs[:, 2 * k:]) - x).abs().max() / x.abs().max()) < 2 ** -16
    assert float(((ws[:, :k] + ws[:, k:2 * k]) - w).abs().div(w.abs() + 1e-30).max()) < 2 ** -15
    got = y.double().cpu()
    err = float((got - want).norm() / want.norm())
    err_bf = float(((x.bfloat16().double() @ w.bfloat16().double().T + b.double()) - want).norm() / want.norm())
    err_f32 = float(((x @ w.T + b).double() - want).norm() / want.norm())
    print(f"bf16x3 linear {m}x{n}x{k}: rel-L2 vs fp64 {err:.2e} (torch fp32 on the CPU {err_f32:.2e}, plain bf16 operands {err_bf:.2e})")
    assert err < 2e-5 and err < 0.01 * err_bf
    # ... and against the CPU restatement of the SAME arithmetic (oracle/bf16x3.py): only the accumulation order differs
    from oracle import bf16x3
    ref3 = bf16x3.linear_x3(x, w, b).double()
    assert torch.equal(x3.cpu(), bf16x3.split3_activation(x)) and torch.equal(w3.cpu(), bf16x3.split3_weight(w))
    assert float((got - ref3).norm() / ref3.norm()) < 2e-6
    row = (got - want).norm(dim=1) / want.norm(dim=1)
    assert float(row.max()) < 5e-5  # per row: the wide per-row scales do not leak into each other


@pytest.mark.parametrize("batch,heads,s_pad,n_valid", [(2, 2, 128, 100), (1, 3, 256, 256), (1, 2, 1408, 1370), (1, 1, 128, 1),
                                                        (3, 12, 1408, 1370)])
@pytest.mark.parametrize("spike", [0.0, 1.5])
def test_attention_f32x3_vs_fp64(L, batch, heads, s_pad, n_valid, spike):
    """bf16x3 attention of the `--fp32_matmul high` extractor: fp32 q, k, v with a wide range, fp64 reference, and (spike)
    one key row aligned with a few queries so that the running max jumps late (the rescale branch).  Must sit within 1e-4
    of fp64 -- the exact-fp32 kernel is printed beside it."""
    torch.manual_seed(s_pad + heads)
    dim = heads * 64
    q = torch.randn(batch, s_pad, heads, 64) * 1.5
    k = torch.randn(batch, s_pad, heads, 64) + torch.linspace(-1, 1, 64)
    v = torch.randn(batch, s_pad, heads, 64) * torch.linspace(0.5, 1.5, 64) * torch.exp(torch.randn(batch, s_pad, 1, 1))
    if spike and n_valid > 70:
        key = min(n_valid - 1, 64 * 3 + 17)
        k[:, key] = 0.0
        for qi in (3, 50, n_valid - 1):
            k[:, key] += q[:, qi] * spike / 2.25
    att = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q.double() * 0.125, k.double()[:, :n_valid]), -1)
    want = torch.einsum("bhqk,bkhd->bqhd", att, v.double()[:, :n_valid]).reshape(batch, s_pad, dim)
    qkv = torch.cat([q.reshape(batch * s_pad, dim), k.reshape(batch * s_pad, dim), v.reshape(batch * s_pad, dim)],
                    1).contiguous().to(DEV)
    out = torch.empty((batch * s_pad, dim), device=DEV, dtype=torch.float32)
    exact = torch.empty_like(out)
    scratch = torch.zeros(int(L.dvt_vit_attention_x3_scratch_bytes(batch, heads, s_pad)), device=DEV, dtype=torch.uint8)
    assert L.dvt_vit_attention_x3(qkv.data_ptr(), out.data_ptr(), scratch.data_ptr(), batch, heads, s_pad, n_valid, _s()) == 0
    assert L.dvt_vit_attention_f32(qkv.data_ptr(), exact.data_ptr(), batch, heads, s_pad, n_valid, _s()) == 0
    torch.cuda.synchronize()
    got, ex = out.double().reshape(batch, s_pad, dim).cpu(), exact.double().reshape(batch, s_pad, dim).cpu()
    e, e_ex = rel(got[:, :n_valid], want[:, :n_valid]), rel(ex[:, :n_valid], want[:, :n_valid])
    rows = ((got - want)[:, :n_valid].norm(dim=-1) / want[:, :n_valid].norm(dim=-1)).max()
    print(f"bf16x3 attention b{batch} h{heads} n{n_valid} spike {spike}: rel-L2 {e:.2e} (exact-fp32 kernel {e_ex:.2e}), worst row {rows:.2e}")
    # split_out = 1: the same result as the next GEMM's [hi | hi | lo] rows.  hi is bit for bit bf16(out); lo may differ from
    # bf16(out - hi) in its last bit (the compiler contracts o * inv - hi into one fma, i.e. lo is formed from the unrounded
    # product): hi + lo must reproduce out to the split's 2^-16
    out3 = torch.empty((batch * s_pad, 3 * dim), device=DEV, dtype=torch.bfloat16)
    assert L.dvt_vit_attention_x3_presplit(scratch.data_ptr(), out3.data_ptr(), batch, heads, s_pad, n_valid, 1, _s()) == 0
    torch.cuda.synchronize()
    from oracle import bf16x3 as _x3
    rows_valid = torch.arange(batch * s_pad).reshape(batch, s_pad)[:, :n_valid].reshape(-1)
    o3, of = out3.cpu()[rows_valid].float(), out.cpu()[rows_valid]
    assert torch.equal(o3[:, :dim], of.bfloat16().float()) and torch.equal(o3[:, :dim], o3[:, dim:2 * dim])
    assert float(((o3[:, :dim] + o3[:, 2 * dim:]) - of).abs().max() / of.abs().max()) < 2.0 ** -16
    assert _x3.split3_activation(of).shape == o3.shape
    # the CPU restatement of the same three-term arithmetic (one head).  The two differ in WHICH bits the splits of P round
    # away (online softmax against a lagging running max vs the true row max), so they agree to the error class of
    # the method, not tighter: 0.9-1.1e-5 measured
    from oracle import bf16x3
    ref3 = bf16x3.attention_x3(q[0, :n_valid, 0], k[0, :n_valid, 0], v[0, :n_valid, 0], 0.125).double()
    e3 = float((got[0, :n_valid, :64] - ref3).abs().max() / ref3.abs().max())
    assert e3 < 3e-5, e3
    assert e < 5e-5 and float(rows) < 2e-4
    assert bool(torch.isfinite(out[: batch * s_pad].reshape(batch, s_pad, dim)[:, :n_valid]).all())


@pytest.mark.parametrize("knob", [None, -520, -522])  # default | exact-fp32 attention | split kernels instead of split epilogues
@pytest.mark.parametrize("dim,depth,img,stride,n_reg", [(128, 2, 56, 14, 0), (256, 2, 98, 7, 4), (768, 2, 518, 14, 0),
                                                        (768, 12, 518, 14, 0)])
def test_vit_forward_f32x3_vs_oracle(L, dim, depth, img, stride, n_reg, knob):
    """HipViT(dtype="float32", matmul="high"): linear layers through bf16x3, everything else fp32.  Held to the SAME
    fp32-oracle bars as the exact-fp32 extractor except for the rel-L2 bound (1e-4 instead of 2e-5), with an odd batch
    (3 views: 1.5 GEMM tiles of phantom rows at s_pad 1408) and the result of the exact path printed beside it."""
    from dvt_amd.vit import HipViT, random_state_dict
    g0 = img // 14
    sd = random_state_dict(dim, depth, 14, (0 if n_reg else 1) + g0 * g0, seed=dim + 1, well_conditioned=True,
                           n_reg=n_reg)
    x = torch.randn(3, 3, img, img, generator=torch.Generator().manual_seed(3))
    want = ovit.forward_features(sd, x, 14, stride)
    try:
        if knob is not None:
            assert L.dvt_tune_set(1, knob) == 0
        got = HipViT(sd, 14, stride, (img, img), DEV, dtype="float32", matmul="high").forward_features(x.to(DEV)).cpu()
    finally:
        L.dvt_tune_set(1, -521)
        L.dvt_tune_set(1, -523)
    exact = HipViT(sd, 14, stride, (img, img), DEV, dtype="float32").forward_features(x.to(DEV)).cpu()
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    err, err_exact = float((got - want).norm() / want.norm()), float((exact - want).norm() / want.norm())
    cos = F.cosine_similarity(got.reshape(-1, dim), want.reshape(-1, dim), dim=-1)
    bf = HipViT(sd, 14, stride, (img, img), DEV).forward_features(x.to(DEV)).cpu()
    err_bf = float((bf - want).norm() / want.norm())
    print(f"fp32 ViT, bf16x3 (knob {knob}), dim={dim} depth={depth} stride={stride} reg={n_reg}: rel-L2 {err:.2e} "
          f"(exact fp32 {err_exact:.2e}, bf16 extractor {err_bf:.2e}), cos min {cos.min():.8f}")
    assert err < 1e-4 and cos.min() > 0.999999
    assert err < 0.05 * err_bf
    with pytest.raises(Exception):
        HipViT(sd, 14, stride, (img, img), DEV, dtype="bfloat16", matmul="high")


@pytest.mark.parametrize("depth,batch", [(3, 2), (12, 4)])
def test_layernorm_folded_into_gemms(L, depth, batch):
    """LayerNorm folded into the qkv / fc1 GEMMs and the proj / fc2 residual epilogues (dvt_vit_epilogue.h: ln_fold) against
    the LayerNorm kernels (dvt_tune_set(1, -60)) and the fp32 oracle, ViT-B/14 geometry, random LayerNorm affine
    parameters (so that gamma / beta folding is exercised), even batch = whole 256-row tiles."""
    from dvt_amd.vit import HipViT, random_state_dict
    sd = random_state_dict(768, depth, 14, 1370, seed=depth, well_conditioned=True)
    g = torch.Generator().manual_seed(depth)
    for k in list(sd):
        if k.endswith("norm1.weight") or k.endswith("norm2.weight"):
            sd[k] = sd[k] * (1.0 + 0.3 * torch.randn(sd[k].shape, generator=g))
        if k.endswith("norm1.bias") or k.endswith("norm2.bias"):
            sd[k] = sd[k] + 0.2 * torch.randn(sd[k].shape, generator=g)
    x = torch.randn(batch, 3, 518, 518, generator=g)
    want = ovit.forward_features(sd, x[:2], 14, 14)
    vit = HipViT(sd, 14, 14, (518, 518), DEV)
    folded = vit.forward_features(x.to(DEV)).cpu()
    try:
        assert L.dvt_tune_set(1, -60) == 0
        plain = vit.forward_features(x.to(DEV)).cpu()
    finally:
        L.dvt_tune_set(1, -61)
    assert not torch.equal(folded, plain), "the folded path did not run"
    cf = torch.nn.functional.cosine_similarity(folded[:2].reshape(-1, 768), want.reshape(-1, 768), dim=-1)
    cp = torch.nn.functional.cosine_similarity(plain[:2].reshape(-1, 768), want.reshape(-1, 768), dim=-1)
    rel = float((folded - plain).norm() / plain.norm())
    print(f"LN folded (depth {depth}): vs oracle cos mean {cf.mean():.6f} min {cf.min():.6f} (LN kernels: {cp.mean():.6f} / "
          f"{cp.min():.6f}); folded vs kernels rel-L2 {rel:.4f}")
    assert cf.min() > cp.min() - 2e-4 and cf.mean() > cp.mean() - 1e-4 and cf.min() > 0.999
    # an odd batch gets phantom rows up to a whole 256-row tile and takes the same kernels: batching changes nothing
    one = vit.forward_features(x[:1].to(DEV)).cpu()
    assert torch.equal(one, folded[:1])
    three = vit.forward_features(x[:3].to(DEV), max_batch=3).cpu()
    assert torch.equal(three, folded[:3])


def test_vit_large_full_depth(L):
    """BASELINE configs[2] as a configuration: the DINOv2 ViT-L/14 geometry at FULL depth -- 24 blocks, dim 1024, 16
    heads, mlp 4096, 518 x 518 (1370 tokens) -- through the wrapper's own constructor (`vit_large_patch14_dinov2.lvd142m`,
    vit_wrapper.py:15-56), well-conditioned random weights in the timm layout, 2 views, against the fp32 oracle: the bf16
    extractor (per-token cosine) and the fp32 extractor (rel-L2).  Round 3 held 2 of the 24 blocks against the oracle."""
    import warnings

    from dvt_amd.models import PretrainedViTWrapper
    from dvt_amd.vit import HipViT, random_state_dict
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = PretrainedViTWrapper("vit_large_patch14_dinov2.lvd142m", stride=14, allow_random_init=True)
    assert (w.n_output_dims, w.num_blocks, w.last_layer_index, w.patch_size) == (1024, 24, 23, 14)
    sd = random_state_dict(1024, 24, 14, 1370, seed=24, well_conditioned=True)
    x = torch.randn(2, 3, 518, 518, generator=torch.Generator().manual_seed(5))
    stream = []
    want = ovit.forward_features(sd, x, 14, 14, stream_out=stream)
    assert want.shape == (2, 37, 37, 1024) and bool(torch.isfinite(want).all())
    got = HipViT(sd, 14, 14, (518, 518), DEV).forward_features(x.to(DEV)).cpu()
    cos = F.cosine_similarity(got.reshape(-1, 1024), want.reshape(-1, 1024), dim=-1)
    err = float((got - want).norm() / want.norm())
    print(f"ViT-L/14 FULL depth (24 blocks) bf16 extractor vs fp32 oracle: cos mean {cos.mean():.6f} min {cos.min():.6f} "
          f"rel-L2 {err:.4f}; residual stream |x| mean before the final norm {float(stream[0].abs().mean()):.0f}")
    assert got.shape == want.shape and cos.min() > 0.999 and err < 3e-2
    got32 = HipViT(sd, 14, 14, (518, 518), DEV, dtype="float32").forward_features(x.to(DEV)).cpu()
    err32 = float((got32 - want).norm() / want.norm())
    cos32 = F.cosine_similarity(got32.reshape(-1, 1024), want.reshape(-1, 1024), dim=-1)
    print(f"ViT-L/14 FULL depth fp32 extractor vs fp32 oracle: rel-L2 {err32:.2e}, cos min {cos32.min():.8f}")
    assert err32 <= 1e-5 and cos32.min() > 0.999999


def test_vit_large_launch_beyond_2p31_elements(L):
    """the default launch cap (400 views) gives a ViT-L/14 launch of 395 views an fc1 output of 395 x 1408 x 4096 =
    2.28e9 elements and a qkv output of 1.7e9 -- beyond 2^31, where every index must be 64-bit -- and no test ran there (the
    full-depth test uses 2 views).  Two blocks of the ViT-L geometry on 395 views in ONE launch against the same views in
    five launches of 79 (every intermediate below 2^31 elements): results must not depend on the batching.  The fold of the
    LayerNorm statistics sums 64-column partials in a fixed order per row, so the two runs agree to the last bit."""
    from dvt_amd.vit import HipViT, random_state_dict
    sd = random_state_dict(1024, 2, 14, 1370, seed=7, well_conditioned=True)
    n = 395
    x = torch.randn(n, 3, 518, 518, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))
    vit = HipViT(sd, 14, 14, (518, 518), DEV)
    assert vit.launch_plan(n, 400) == [n] and n * vit.cfg.s_pad * vit.cfg.mlp_dim > 2 ** 31
    big = vit.forward_features(x, max_batch=400)
    torch.cuda.synchronize()
    assert max(vit.launch_plan(n, 79)) <= 79
    small = vit.forward_features(x, max_batch=79)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(big).all())
    diff = float((big - small).abs().max())
    print(f"ViT-L/14 geometry, 2 blocks: 1 launch of {n} views vs launches of <= 79: max |diff| {diff:.3e}")
    assert diff == 0.0
    # and the last view of the big launch against the oracle (the rows with the largest offsets)
    want = ovit.forward_features(sd, x[-1:].cpu(), 14, 14)
    cos = F.cosine_similarity(big[-1:].cpu().reshape(-1, 1024), want.reshape(-1, 1024), dim=-1)
    assert cos.min() > 0.999, float(cos.min())


def test_gemm_staggered_start_does_not_change_results(L):
    """dvt_tune_set(1, -700 - pct): the first round of 8p workgroups starts spread over pct % of a tile time (a measured null,
    profiles/r05/r05c_*; default off).  It only delays workgroups: the output must equal the default launch bit for bit, on a
    launch of more than two rounds of tiles (below that the knob is not applied)."""
    m, n, k = 256 * 72, 2304, 768  # 72 x 9 = 648 tiles
    g = torch.Generator(device=DEV).manual_seed(3)
    x = (torch.rand(m, k, device=DEV, generator=g) * 2 - 1).bfloat16()
    w = ((torch.rand(n, k, device=DEV, generator=g) * 2 - 1) / k ** 0.5).bfloat16()
    b = torch.randn(n, device=DEV, generator=g)
    outs = {}
    try:
        for pct in (0, 100, 250):
            assert L.dvt_tune_set(1, -700 - pct) == 0
            y = torch.full((m, n), float("nan"), device=DEV, dtype=torch.bfloat16)
            assert L.dvt_vit_gemm_bias(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), m, n, k, _s()) == 0
            torch.cuda.synchronize()
            outs[pct] = y
    finally:
        L.dvt_tune_set(1, -700)
    assert bool(torch.isfinite(outs[0].float()).all())
    for pct in (100, 250):
        assert torch.equal(outs[pct].view(torch.int16), outs[0].view(torch.int16)), pct


def test_product_library_rejects_lab_knobs(L):
    """the product library carries no superseded / experimental / timing kernel, and dvt_tune_set refuses every
    value that would have selected one (before: `dvt_tune_set(1, -301)` made a product entry point return wrong numbers with
    rc 0).  What it accepts are the schedules the tests above hold against the references."""
    BADARG = -1
    assert L.dvt_vit_is_lab_build() == 0
    for v in (0, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13,   # superseded / experimental GEMM schedules
              -200, -203, -300, -301, -303, -309,     # 4w tiles per workgroup, ablation masks / timing builds
              -364, -399, -400, -410, -499,           # retired 8q values
              -500, -501, -503, -510, -511, -589,     # round-2 attention loop, other schedule masks
              -600, -616):                            # 4w grid
        assert L.dvt_tune_set(1, v) == BADARG, v
    assert L.dvt_vit_debug_buffer(None) == BADARG
    for v in (4, 3, 1, -502, -525, -61, -60, -51, -50, -104, -100, 2400, 4800, -521, -523, GEMM_DEFAULT):
        assert L.dvt_tune_set(1, v) == 0, v
    assert L.dvt_tune_set(1, -61) == 0 and L.dvt_tune_set(1, 4800) == 0 and L.dvt_tune_set(1, GEMM_DEFAULT) == 0
