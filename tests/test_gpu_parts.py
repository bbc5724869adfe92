"""Element-level parity of the exact-fp32 trainer kernels against fp64, one kernel at a time (include/dvt_parts.h).

The step tests (test_gpu_stage2.py, test_gpu_stage3.py, test_gpu_stage3_grid.py) hold a relative L2 error per gradient
tensor; that cannot see one wrong tile edge, a k-tile lost by a short last k-split, a padded query block or the idle lanes
of a 384-wide row.  Here every kernel behind the component entry points is compared ELEMENT BY ELEMENT -- nothing sampled,
nothing skipped -- with the plain fp64 references of tests/parts_reference.py, at the smallest shapes at which each path can
still go wrong.  Tolerances are per element, computed in fp64 from the inputs (never from the kernel under test):

  contractions            (K + S + 4) u (|A| . |B|) (+ 2 u |bias|; a prefilled C counts as one more term), S = k-splits
  function of one         that bound through the function's derivative to first order, plus the function's own rounding:
                          c u |ref| for the softmax of the attention logits and for scale P (.) (acc - D) (c from the
                          float32 CPU evaluation of the function on the fp32-rounded contraction).  The two epilogues
                          that CANCEL get their terms' magnitudes instead of |ref|: 2 u (|C0| + |gamma v|) for the residual
                          C0 + gamma v, and c L u mag of the elementwise GELU for the GELU epilogue -- for v < 0 gelu(v) is
                          v / 2 times the small difference 1 + erf(v / sqrt 2), and an fp32 1 + erf is wrong by u in
                          ABSOLUTE terms whatever library computes it (at v = -3 that is 400 u |gelu(v)|; a c measured
                          against |ref| would come out near 10^4 and loosen every other element by that factor)
  row / elementwise       c L u mag, c = max(1, 4 c_ref), c_ref measured in float32 CPU torch on the same inputs

Outputs are NaN before the call (or hold known values where the kernel accumulates, which the reference adds); a sentinel
band lies behind each output and sentinels fill the gaps of strided outputs (ldc > N, head slices of [R][3C]); afterwards
every band and gap must hold the sentinel bit for bit.  Rows and columns a kernel defines as padding must be exactly 0.0.
Inputs the kernel must not read (gaps of lda > K, padded token rows) are NaN.  Knobs are set inside try / finally.

Worst err / tol per kernel, measured on MI355X at commit 4f2de9e + this change (python -m pytest -m gpu -s prints them):
  add_ln.mean 0.004,  add_ln.rstd 0.002,  add_ln.sum 0.250,  add_ln.xn 0.002
  attn_rows.backward 0.063,  attn_rows.forward 0.037,  attn_rows.rowsum 0.083,  gelu.a 0.258
  gelu_bwd.da 0.211,  gemm_ex.batched_dS 0.067,  gemm_ex.batched_dv 0.030,  gemm_ex.batched_pv 0.032
  gemm_ex.batched_qk 0.078,  gemm_ex.colsum 0.018,  gemm_ex.layout0 0.047,  gemm_ex.layout1 0.026
  gemm_ex.layout2 0.020,  lin_bwd.db 0.015,  lin_bwd.dw 0.064,  lin_bwd.dx 0.033
  lin_fwd 0.047,  linear_big.epi0 0.115,  linear_big.epi1 0.124,  linear_big.epi2 0.488
  linear_big.fallback 0.083,  ln_bwd.dbeta 0.250,  ln_bwd.dgamma 0.250,  ln_bwd.dx 0.005
  loss_rows.dout 0.005,  loss_rows.loss 0.000,  loss_rows.out 0.250,  ls_add_ln.mean 0.006
  ls_add_ln.rstd 0.001,  ls_add_ln.sum 0.250,  ls_add_ln.xn 0.004,  ls_bwd.df 0.250
  ls_bwd.dls 0.015,  pos_grad.dpos 0.252,  rowdot.D 0.009,  s3_embed.x 0.250
  s3_embed_bwd.dpos 0.250,  s3_embed_bwd.dprefix 0.250,  softmax.P 0.204,  softmax_bwd.dS 0.023
All are below 0.5.  The 0.25 of the two-term sums (add_ln.sum, ls_bwd.df, s3_embed.x, ...) is ONE rounding, u |v|, against
L u mag = 2 u mag with c = 2; linear_big.epi2 (0.49) is the one rounding of C0 + gamma v against 2 u (|C0| + |gamma v|).
"""
import ctypes as C

import pytest
import torch

from tests import parts_reference as pr

pytestmark = pytest.mark.gpu
DEV = "cuda"
BADARG = -1
U = pr.U
SENT = 0x5A5A5A5A
BAND = 8192
NAN = float("nan")
D64 = torch.float64
RATIOS = {}


def _s():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def L(built_lib):
    return built_lib


class Knob:
    """dvt_tune_set(key, value) for the block, `default` restored whatever happens."""

    def __init__(self, L, key, value, default):
        self.L, self.key, self.value, self.default = L, key, value, default

    def __enter__(self):
        assert self.L.dvt_tune_set(self.key, self.value) == 0

    def __exit__(self, *exc):
        assert self.L.dvt_tune_set(self.key, self.default) == 0


def stages(L, ns):
    return Knob(L, 4, ns, 2)  # LDS ring depth of dvt_gemm_f32_ex and the 64 x 64 fallback of dvt_linear_fwd_big (default 2)


def s2_mask(L, mask):
    return Knob(L, 18, mask, 63)


class Buf:
    """An output of logical `shape` (gaps included) with a sentinel band behind it.  `owned` selects the part the kernel may
    write (default: all of it); that part starts as NaN or as `fill`, everything else holds the sentinel."""

    def __init__(self, shape, owned=None, fill=None, offset=0):
        n = 1
        for v in shape:
            n *= v
        self.raw = torch.full((n + BAND,), SENT, device=DEV, dtype=torch.int32)
        self.full = self.raw.view(torch.float32)[:n].view(shape)
        self.mask = torch.zeros(n + BAND, device=DEV, dtype=torch.bool)
        mv = self.mask[:n].view(shape)
        (owned(mv) if owned else mv)[...] = True
        self.out = owned(self.full) if owned else self.full
        if fill is None:
            self.out[...] = NAN
        else:
            self.out.copy_(fill.to(DEV))
        self.offset = offset

    def ptr(self):
        return self.full.data_ptr() + 4 * self.offset

    def check(self, what):
        bad = ((self.raw != SENT) & ~self.mask).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.numel()} sentinel elements overwritten, first at offset {int(bad[0])}"

    def untouched(self, what):
        self.check(what)
        assert bool(self.out.isnan().all()), f"{what}: a refused call wrote its output"


def dev(t):
    return t.to(DEV).contiguous()


def mem(t, ld):
    """t [rows][cols] laid out with leading dimension ld >= cols; the gap is NaN (never read)."""
    m = torch.full((t.shape[0], ld), NAN, device=DEV)
    m[:, :t.shape[1]] = t.to(DEV)
    return m


def compare(got, ref, tol, what, kernel):
    """|got - ref| <= tol element by element (NaN fails); records and prints the worst err / tol of `kernel`."""
    got = got.detach().to("cpu", D64).reshape(ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= tol)
    ratio = float((err / tol.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max()) if ref.numel() else 0.0
    print(f"err/tol {what}: {ratio:.3f}")
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), ratio)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements out of tolerance; first at {idx}: got "
                             f"{float(got.flatten()[i])!r} want {float(ref.flatten()[i])!r} tol {float(tol.flatten()[i]):.3g}")


def check_rows(kernel, what, ref, inp, got):
    """Row / elementwise kernel: every output in `got` against ref in fp64 within c L u mag."""
    r64 = ref(pr.cast(inp, D64))
    tol = pr.row_tol(r64, pr.yardstick(ref, inp))
    for k, g in got.items():
        compare(g, r64[k][0], tol[k], f"{what} {k}", f"{kernel}.{k}")
    return r64


def zeros_exactly(t, what):
    assert bool((t == 0).all()), f"{what}: {int((t != 0).sum())} padding elements are not exactly 0"


# ============================================================================================ dvt_parts_gemm_ex, unbatched
def gemm_ex_call(L, **kw):
    g = pr_struct(**kw)
    return L.dvt_parts_gemm_ex(C.byref(g), _s())


def pr_struct(**kw):
    from dvt_amd._lib import PartsGemmEx
    g = PartsGemmEx()
    for k, v in kw.items():
        setattr(g, k, v)
    return g


@pytest.mark.parametrize("ns", [2, 3])
@pytest.mark.parametrize("layout,M,N,K,bias,acc", pr.GEMM_EX_CASES)
def test_gemm_ex_unbatched(L, layout, M, N, K, bias, acc, ns):
    """The 64 x 64 LDS-DMA kernel at partial tiles (M = 100, N = 72: rows clamped at the source, masked at the store), one and
    three k-tiles (an odd count for both ring depths), lda > K, ldc > N, and the uneven k-split of the accumulating weight
    gradient: K = 576 is 9 k-tiles in 2 splits of 5 and 4 (K = 128: one split)."""
    i = pr.gemm_inputs(M, N, K, pr.seed_of("gemm", M, N, K))
    A, Bm = i["A"][0], i["Bm"][0]
    splits, tiles = pr.ex_splits(M, N, K, acc)
    if (layout, K) == (2, 576):
        assert (splits, tiles) == (2, [5, 4])
    if (layout, K) == (2, 128):
        assert (splits, tiles) == (1, [2])
    ldc = N + 5
    if layout == 0:
        a, b = mem(A, K + 8), mem(Bm.t(), K + 4)
    elif layout == 1:
        a, b = mem(A, K + 4), mem(Bm, N + 4)
    else:
        a, b = mem(A.t(), M + 4), mem(Bm, N + 4)
    c = Buf((M, ldc), owned=lambda v: v[:, :N], fill=i["C0"][0] if acc else None)
    cs = Buf((M,), fill=i["colsum0"])
    bv = dev(i["bias"])
    with stages(L, ns):
        rc = gemm_ex_call(L, layout=layout, A=a.data_ptr(), B=b.data_ptr(), C=c.ptr(), M=M, N=N, K=K, lda=a.shape[1], ldb=b.shape[1],
                          ldc=ldc, bias=bv.data_ptr() if bias else None, colsum=cs.ptr() if acc else None, accumulate=int(acc))
        torch.cuda.synchronize()
    assert rc == 0
    what = f"gemm_ex layout {layout} {M}x{N}x{K} stages {ns}"
    c.check(what)
    cs.check(what + " colsum")
    ref, mag, csr, csm = pr.ref_gemm(pr.cast(i, D64), bias=bias, accumulate=acc)
    compare(c.out, ref[0], pr.gemm_tol(mag[0], K, splits, i["bias"].double() if bias else None), what, f"gemm_ex.layout{layout}")
    if acc:
        compare(cs.out, csr, (K + splits + 4) * U * csm, what + " colsum", "gemm_ex.colsum")
    else:
        assert torch.equal(cs.out.cpu(), i["colsum0"])  # colsum belongs to layout 2 only


# ============================================================================================== dvt_parts_gemm_ex, batched
NB0, NB1, TP, CH = 2, 3, 128, 192  # the trainers' strides for 3 heads of 64 and tokens_pad 128


def scatter_heads(buf, t, col0):
    """t [NB0 * NB1][TP][64] into the head slices (columns col0 + 64 h) of buf [NB0 * TP][ld]."""
    v = buf.view(NB0, TP, -1)
    for b0 in range(NB0):
        for h in range(NB1):
            v[b0, :, col0 + 64 * h:col0 + 64 * h + 64] = t[b0 * NB1 + h].to(DEV)


def gather_heads(buf, col0):
    v = buf.view(NB0, TP, -1)
    return torch.stack([v[b0, :, col0 + 64 * h:col0 + 64 * h + 64] for b0 in range(NB0) for h in range(NB1)])


@pytest.mark.parametrize("ns", [2, 3])
@pytest.mark.parametrize("kind", ["qk", "dS", "pv", "dv"])
def test_gemm_ex_batched(L, kind, ns):
    """The six (image, head)-batched attention products' forms: qk = q k^T (layout 0, K = 64: the small-k kernel), dS = the same
    kernel with the softmax-backward epilogue oscale * smul (.) (acc - rowsub), pv = P v (layout 1) into a head slice of [R][3C],
    dv = P^T d ao (layout 2) into the v slice of [R][3C]; the other columns of [R][3C] hold sentinels."""
    nb = NB0 * NB1
    M, N, K = {"qk": (TP, TP, 64), "dS": (TP, TP, 64), "pv": (TP, 64, TP), "dv": (TP, 64, TP)}[kind]
    i = pr.gemm_inputs(M, N, K, pr.seed_of("gemm_b", kind), nb=nb)
    A, Bm = i["A"], i["Bm"]
    g = pr.gen(pr.seed_of("gemm_b_smul", kind))
    qkv = torch.full((NB0 * TP, 3 * CH), NAN, device=DEV)
    rc_buf = torch.full((NB0 * TP, CH), NAN, device=DEV)
    pp = (NB1 * TP * TP, TP * TP)
    q3, r1 = (TP * 3 * CH, 64), (TP * CH, 64)
    kw = dict(M=M, N=N, K=K, nb0=NB0, nb1=NB1)
    smul = rowsub = None
    if kind in ("qk", "dS"):
        if kind == "qk":
            scatter_heads(qkv, A, 0)
            kw.update(A=qkv.data_ptr(), lda=3 * CH, sA0=q3[0], sA1=q3[1])
        else:
            scatter_heads(rc_buf, A, 0)
            kw.update(A=rc_buf.data_ptr(), lda=CH, sA0=r1[0], sA1=r1[1])
            smul, rowsub = pr.randn(g, nb, M, N), pr.randn(g, nb, M)
            sm_d, rs_d = dev(smul), dev(rowsub)
            kw.update(smul=sm_d.data_ptr(), rowsub=rs_d.data_ptr(), oscale=0.125)
        col0 = CH if kind == "qk" else 2 * CH
        scatter_heads(qkv, Bm.transpose(1, 2), col0)
        c = Buf((nb, M, N))
        kw.update(layout=0, B=qkv.data_ptr() + 4 * col0, ldb=3 * CH, sB0=q3[0], sB1=q3[1], C=c.ptr(), ldc=N, sC0=pp[0], sC1=pp[1])
        got = lambda: c.out
    elif kind == "pv":
        a = dev(A)
        scatter_heads(qkv, Bm, 2 * CH)
        c = Buf((NB0 * TP, 3 * CH), owned=lambda v: v[:, :CH])
        kw.update(layout=1, A=a.data_ptr(), lda=TP, sA0=pp[0], sA1=pp[1], B=qkv.data_ptr() + 4 * 2 * CH, ldb=3 * CH, sB0=q3[0],
                  sB1=q3[1], C=c.ptr(), ldc=3 * CH, sC0=q3[0], sC1=q3[1])
        got = lambda: gather_heads(c.full, 0)
    else:
        a = dev(A.transpose(1, 2))  # [K][M] in memory
        scatter_heads(rc_buf, Bm, 0)
        c = Buf((NB0 * TP, 3 * CH), owned=lambda v: v[:, 2 * CH:], offset=2 * CH)
        kw.update(layout=2, A=a.data_ptr(), lda=TP, sA0=pp[0], sA1=pp[1], B=rc_buf.data_ptr(), ldb=CH, sB0=r1[0], sB1=r1[1],
                  C=c.ptr(), ldc=3 * CH, sC0=q3[0], sC1=q3[1])
        got = lambda: gather_heads(c.full, 2 * CH)
    with stages(L, ns):
        rc = gemm_ex_call(L, **kw)
        torch.cuda.synchronize()
    assert rc == 0
    what = f"gemm_ex batched {kind} stages {ns}"
    c.check(what)
    ref, mag, _, _ = pr.ref_gemm(pr.cast(i, D64))
    tol = pr.gemm_tol(mag, K)
    if kind == "dS":
        ref, tol = pr.pmul_tol(0.125, smul.double(), ref, mag, rowsub.double()[..., None].expand_as(ref))
    compare(got(), ref, tol, what, f"gemm_ex.batched_{kind}")


def test_gemm_ex_refusals(L):
    """Every refusal is decided on the host before any launch: DVT_E_BADARG, outputs untouched."""
    a = torch.zeros(256, 256, device=DEV)
    b = torch.zeros(256, 256, device=DEV)
    sm = torch.zeros(2, 128, 128, device=DEV)
    rs = torch.zeros(2, 128, device=DEV)
    ok = dict(layout=0, A=a.data_ptr(), B=b.data_ptr(), M=64, N=64, K=64, lda=256, ldb=256, ldc=64)
    batched = dict(nb0=2, nb1=1, sA0=64 * 256, sB0=64 * 256, sC0=64 * 64)
    bad = {"K % 64": dict(ok, K=96),
           "layout 2 with M % 64": dict(ok, layout=2, M=96, N=64),
           "layout 1 with N % 64": dict(ok, layout=1, N=96, ldc=96),
           "lda % 4": dict(ok, lda=254),
           "ldb % 4": dict(ok, ldb=254),
           "smul with K > 64": dict(ok, K=128, smul=sm.data_ptr(), rowsub=rs.data_ptr(), oscale=1.0, **batched),
           "smul unbatched": dict(ok, smul=sm.data_ptr(), rowsub=rs.data_ptr(), oscale=1.0),
           "smul without rowsub": dict(ok, smul=sm.data_ptr(), oscale=1.0, **batched),
           "smul with accumulate": dict(ok, smul=sm.data_ptr(), rowsub=rs.data_ptr(), accumulate=1, **batched),
           "layout 3": dict(ok, layout=3),
           "K = 0": dict(ok, K=0),
           "A = NULL": dict(ok, A=None)}
    for what, kw in bad.items():
        c = Buf((2, 128, 128))
        rc = gemm_ex_call(L, C=c.ptr(), **kw)
        torch.cuda.synchronize()
        assert rc == BADARG, what
        c.untouched(what)
    c = Buf((64, 64))  # and the valid form of the same call runs
    assert gemm_ex_call(L, C=c.ptr(), **ok) == 0
    torch.cuda.synchronize()
    zeros_exactly(c.out, "0 . 0")


# ============================================================================================ dvt_parts_linear_big_epi
def big_epi_case(L, m, n, k, epi, bias, kernel):
    i = pr.gemm_inputs(m, n, k, pr.seed_of("gemm", m, n, k))
    x, w = dev(i["A"][0]), dev(i["Bm"][0].t())
    bv, gm = dev(i["bias"]), dev(i["gamma"])
    y = Buf((m, n), fill=i["C0"][0] if epi == 2 else None)
    rc = L.dvt_parts_linear_big_epi(x.data_ptr(), w.data_ptr(), bv.data_ptr() if bias else None, y.ptr(), m, n, k, epi,
                                    gm.data_ptr() if epi == 2 else None, _s())
    torch.cuda.synchronize()
    assert rc == 0
    what = f"linear_big_epi {m}x{n}x{k} epi {epi} bias {int(bias)}"
    y.check(what)
    j = pr.cast(i, D64)
    v, mag, _, _ = pr.ref_gemm(j, bias=bias)
    v, tv = v[0], pr.gemm_tol(mag[0], k, 1, j["bias"] if bias else None)
    if epi == 0:
        ref, tol = v, tv
    elif epi == 1:
        ref, gmag, gd = pr.gelu_parts(v)
        c = max(1.0, 4.0 * pr.yardstick(pr.ref_gelu, {"h": v.float()})["a"])
        tol = gd * tv + c * 2 * U * gmag
    else:
        c0, gam = j["C0"][0], j["gamma"]
        ref = c0 + gam * v
        tol = gam.abs() * tv + 2 * U * (c0.abs() + (gam * v).abs())
    compare(y.out, ref, tol, what, kernel)


@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("m,n,k", pr.BIG_EPI_SHAPES)
def test_linear_big_epi(L, m, n, k, epi):
    """The 128 x 128 x 32 tile with one and three k-tiles (both buffers of its 2-stage ring, an odd count), one and two tiles
    either way, plain / GELU / residual (onto known C values)."""
    big_epi_case(L, m, n, k, epi, True, f"linear_big.epi{epi}")


@pytest.mark.parametrize("epi", [0, 1, 2])
def test_linear_big_epi_without_bias(L, epi):
    big_epi_case(L, 128, 256, 96, epi, False, f"linear_big.epi{epi}")


@pytest.mark.parametrize("ns", [2, 3])
@pytest.mark.parametrize("m,n,k", pr.BIG_FALLBACK_SHAPES)
def test_linear_big_fallbacks(L, m, n, k, ns):
    """Shapes the 128 x 128 tile does not take: m = 192 goes to the 64 x 64 LDS-DMA kernel, k = 36 (no whole 64-tile) to the
    register-staged kernel."""
    with stages(L, ns):
        big_epi_case(L, m, n, k, 0, True, "linear_big.fallback")


def test_linear_big_epi_refusals(L):
    x = torch.zeros(192, 64, device=DEV)
    w = torch.zeros(128, 64, device=DEV)
    gm = torch.zeros(128, device=DEV)
    for what, args in {"epi 1 off the 128-tile": (192, 128, 64, 1, None), "epi 2 off the 128-tile": (192, 128, 64, 2, gm.data_ptr()),
                       "epi 2 without gamma": (128, 128, 64, 2, None), "epi 3": (128, 128, 64, 3, None),
                       "k % 4": (128, 128, 30, 0, None)}.items():
        y = Buf((192, 128))
        m, n, k, epi, g = args
        assert L.dvt_parts_linear_big_epi(x.data_ptr(), w.data_ptr(), None, y.ptr(), m, n, k, epi, g, _s()) == BADARG, what
        torch.cuda.synchronize()
        y.untouched(what)


# ================================================== launches that cross the units of the fp32 GEMM (csrc/dvt_gemm_f32_dev.h)
# dvt_linear_fwd_big -> the ring (dvt_gemm_f32_glds.hip) and -> the register-staged kernel (dvt_gemm_f32.hip) are crossed by
# test_linear_big_fallbacks above, the batched small-k kernel beside the ring (body in the shared header), with and without the
# softmax-backward epilogue and at both ring depths, by test_gemm_ex_batched[qk / dS].  The two below are the rest.
def test_linear_big_tile_switched_off(L):
    """dvt_tune_set(4, 10) -- decoded by the 128 x 128 unit -- sends the shape its tile would take (128 x 128 x 32) to another
    unit: k = 32 is no whole 64-tile, so to the register-staged kernel.  Tolerance: test_linear_big_fallbacks' (big_epi_case)."""
    with Knob(L, 4, 10, 11):
        big_epi_case(L, 128, 128, 32, 0, True, "linear_big.fallback")


def test_fit_linear_on_the_ring(L):
    """dvt_tune_set(5, 64): dvt_linear_fwd / dvt_linear_bwd (the fit's unit) launch the ring of dvt_gemm_f32_glds.hip through
    its launcher, at m = n = k = 64: the smallest shape the ring takes in all three layouts (forward, dgrad with the ReLU mask,
    atomically accumulated wgrad with the bias gradient).  Against float64 products of the same inputs, with the bounds of
    tests/test_gpu_kernels.py::test_linear_fwd_bwd_vs_torch: 2e-6 of the largest element forward and dgrad, 2e-5 wgrad and bias."""
    g = pr.gen(pr.seed_of("fit_ring", 64))
    x, w, b, dy, mask = pr.randn(g, 64, 64), pr.randn(g, 64, 64) / 8, pr.randn(g, 64), pr.randn(g, 64, 64), pr.randn(g, 64, 64)
    X, W, B_, DY, MK = dev(x), dev(w), dev(b), dev(dy), dev(mask)
    y, dx = Buf((64, 64)), Buf((64, 64))
    dw, db = Buf((64, 64), fill=torch.zeros(64, 64)), Buf((64,), fill=torch.zeros(64))
    with Knob(L, 5, 64, 32):
        rc_f = L.dvt_linear_fwd(X.data_ptr(), W.data_ptr(), B_.data_ptr(), y.ptr(), 64, 64, 64, 1, _s())
        rc_b = L.dvt_linear_bwd(DY.data_ptr(), X.data_ptr(), W.data_ptr(), dw.ptr(), db.ptr(), dx.ptr(), MK.data_ptr(), 64, 64, 64, _s())
        torch.cuda.synchronize()
    assert rc_f == 0 and rc_b == 0
    x, w, b, dy = x.double(), w.double(), b.double(), dy.double()
    want = {"y": (x @ w.t() + b).relu(), "dx": (dy @ w) * (mask > 0), "dw": dy.t() @ x, "db": dy.sum(0)}
    for name, buf, bound in (("y", y, 2e-6), ("dx", dx, 2e-6), ("dw", dw, 2e-5), ("db", db, 2e-5)):
        buf.check(f"fit on the ring {name}")
        err = float((buf.out.double().cpu().reshape(want[name].shape) - want[name]).abs().max() / want[name].abs().max())
        print(f"fit on the ring {name}: relative error {err:.3g}")
        assert err < bound, name


# =================================================================================== dvt_parts_lin_fwd / dvt_parts_lin_bwd
def big_wgrad_taken(mask, R, n, k):
    return bool(mask & 4) and R % 32 == 0 and n % 128 == 0 and k % 128 == 0


@pytest.mark.parametrize("mask", pr.LIN_MASKS)
@pytest.mark.parametrize("R,n,k", pr.LIN_SHAPES)
def test_lin_fwd(L, R, n, k, mask):
    i = pr.gemm_inputs(R, n, k, pr.seed_of("gemm", R, n, k))
    x, w, bv = dev(i["A"][0]), dev(i["Bm"][0].t()), dev(i["bias"])
    y = Buf((R, n))
    with s2_mask(L, mask):
        rc = L.dvt_parts_lin_fwd(x.data_ptr(), w.data_ptr(), bv.data_ptr(), y.ptr(), R, n, k, _s())
        torch.cuda.synchronize()
    assert rc == 0
    what = f"lin_fwd {R}x{n}x{k} mask {mask}"
    y.check(what)
    j = pr.cast(i, D64)
    ref, mag, _, _ = pr.ref_gemm(j, bias=True)
    compare(y.out, ref[0], pr.gemm_tol(mag[0], k, 1, j["bias"]), what, "lin_fwd")


@pytest.mark.parametrize("with_dx", [True, False])
@pytest.mark.parametrize("mask", pr.LIN_MASKS)
@pytest.mark.parametrize("R,n,k", pr.LIN_SHAPES)
def test_lin_bwd(L, R, n, k, mask, with_dx):
    """dx = dy . w, dw += dy^T . x, db += colsum(dy) as the trainers call it (wT scratch given with dx), dw and db prefilled.
    R = 128: every product on the 128 x 128 tile at mask 63 / 31 (the data gradient through the transposed weight); R = 544: the
    128 x 128 weight-gradient tile with 17 row-tiles in 2 splits of 9 and 8, the data gradient on the 64 x 64 kernel (544 is no
    multiple of 128); R = 64, k = 64: the 64 x 64 kernels everywhere.  Mask 31 runs the weight gradient on the caller's stream,
    63 on the side stream: only the CALLER'S stream is synchronised, so a missing join shows.  Mask 0 sends the weight gradient
    to the 64 x 64 kernel, which reduces over whole 64-row tiles: R = 544 is refused there, nothing written."""
    g = pr.gen(pr.seed_of("lin_bwd", R, n, k))
    dy, x, w = pr.randn(g, R, n), pr.randn(g, R, k), pr.randn(g, n, k, scale=n ** -0.5)
    dw0, db0 = pr.randn(g, n, k), pr.randn(g, n)
    dyd, xd, wd = dev(dy), dev(x), dev(w)
    dx, dw, db = Buf((R, k)), Buf((n, k), fill=dw0), Buf((n,), fill=db0)
    wT = Buf((k, n))
    if big_wgrad_taken(mask, R, n, k):
        splits, tiles = pr.wgrad_big_splits(R, n, k)
        if R == 544:
            assert (splits, tiles) == (2, [9, 8])
    else:
        splits, _ = pr.ex_splits(n, k, R - R % 64, True)
    with s2_mask(L, mask):
        rc = L.dvt_parts_lin_bwd(dyd.data_ptr(), xd.data_ptr(), wd.data_ptr(), dx.ptr() if with_dx else None, dw.ptr(), db.ptr(),
                                 wT.ptr() if with_dx else None, R, n, k, _s())
        torch.cuda.current_stream().synchronize()
    what = f"lin_bwd {R}x{n}x{k} mask {mask} dx {int(with_dx)}"
    for b in (dx, dw, db, wT):
        b.check(what)
    if R % 64 and not big_wgrad_taken(mask, R, n, k):
        assert rc == BADARG
        dx.untouched(what)
        assert torch.equal(dw.out.cpu(), dw0) and torch.equal(db.out.cpu(), db0)
        return
    assert rc == 0
    dy64, x64, w64 = dy.double(), x.double(), w.double()
    if with_dx:
        compare(dx.out, dy64 @ w64, pr.gemm_tol(dy64.abs() @ w64.abs(), n), what + " dx", "lin_bwd.dx")
    else:
        assert bool(dx.out.isnan().all())
    compare(dw.out, dw0.double() + dy64.t() @ x64, pr.gemm_tol(dw0.double().abs() + dy64.abs().t() @ x64.abs(), R, splits),
            what + " dw", "lin_bwd.dw")
    compare(db.out, db0.double() + dy64.sum(0), (R + splits + 4) * U * (db0.double().abs() + dy64.abs().sum(0)), what + " db",
            "lin_bwd.db")


# ===================================================================================================== dvt_parts_attn_rows
@pytest.mark.parametrize("late", [False, True])
@pytest.mark.parametrize("Tp,T", pr.ATTN_PADS)
def test_attn_rows_forward(L, Tp, T, late):
    """P = softmax(q k^T / 8) over the valid keys, written once: a single valid key, a partial first key tile, one key into the
    second tile, a padded last tile, no padding, one query of the second 128-row block, and a half-padded second block.  `late`:
    the last valid key tops every query's running maximum by about 50, so the running sum is rescaled by 2^-72 at the very end."""
    i = pr.attn_inputs(Tp, T, pr.seed_of("attn", Tp, T, late), late_key=late)
    B, H = i["batch"], i["heads"]
    Cc = 64 * H
    qkv = dev(i["qkv"])
    out = Buf((B, H, Tp, Tp))
    rc = L.dvt_parts_attn_rows(0, qkv.data_ptr(), 3 * Cc, qkv.data_ptr() + 4 * Cc, 3 * Cc, None, None, out.ptr(), B, H, T, Tp,
                               i["scale"], _s())
    torch.cuda.synchronize()
    assert rc == 0
    what = f"attn_rows forward Tp {Tp} T {T} late {int(late)}"
    out.check(what)
    j = pr.cast(i, D64)
    _, z, _ = pr.ref_attn_fwd(j)
    c = max(1.0, 4.0 * pr.softmax_cref(z.float()))
    P, tol = pr.attn_fwd_tol(j, c)
    got = out.out.cpu()
    zeros_exactly(got[:, :, T:], what + " padded query rows")
    zeros_exactly(got[:, :, :, T:], what + " padded key columns")
    compare(got, P, tol, what, "attn_rows.forward")
    rowsum = got[:, :, :T].double().sum(-1)
    worst = float((rowsum - 1.0).abs().max())
    print(f"err/tol {what} row sums: {worst / ((T + 4) * U):.3f}")
    RATIOS["attn_rows.rowsum"] = max(RATIOS.get("attn_rows.rowsum", 0.0), worst / ((T + 4) * U))
    assert worst <= (T + 4) * U


@pytest.mark.parametrize("Tp,T", [(128, 100), (256, 129)])
def test_attn_rows_backward(L, Tp, T):
    """dS = scale P (.) (d ao v^T - D) with P from the fp64 softmax rounded to fp32 (its padding zeros kept) and random D."""
    i = pr.attn_bwd_inputs(Tp, T, pr.seed_of("attn_bwd", Tp, T))
    B, H = i["batch"], i["heads"]
    Cc = 64 * H
    qkv, dao, P, Dd = dev(i["qkv"]), dev(i["dao"]), dev(i["P"]), dev(i["D"])
    out = Buf((B, H, Tp, Tp))
    rc = L.dvt_parts_attn_rows(1, dao.data_ptr(), Cc, qkv.data_ptr() + 4 * 2 * Cc, 3 * Cc, P.data_ptr(), Dd.data_ptr(), out.ptr(), B,
                               H, T, Tp, i["scale"], _s())
    torch.cuda.synchronize()
    assert rc == 0
    what = f"attn_rows backward Tp {Tp} T {T}"
    out.check(what)
    dS, tol = pr.attn_bwd_tol(pr.cast(i, D64))
    got = out.out.cpu()
    zeros_exactly(got[:, :, T:], what + " padded query rows")
    zeros_exactly(got[:, :, :, T:], what + " padded key columns")
    compare(got, dS, tol, what, "attn_rows.backward")


def test_attn_rows_refusals(L):
    q = torch.zeros(256, 384, device=DEV)
    out = Buf((1, 2, 128, 128))
    for what, (mode, ldk, T, Tp, P) in {"Tp % 128": (0, 384, 64, 64, None), "T > Tp": (0, 384, 129, 128, None), "T = 0": (0, 384, 0, 128, None),
                                        "ld_key % 4": (0, 382, 100, 128, None), "mode 1 without P": (1, 384, 100, 128, None),
                                        "mode 2": (2, 384, 100, 128, None)}.items():
        rc = L.dvt_parts_attn_rows(mode, q.data_ptr(), 384, q.data_ptr() + 512, ldk, P, None, out.ptr(), 1, 2, T, Tp, 0.125, _s())
        torch.cuda.synchronize()
        assert rc == BADARG, what
        out.untouched(what)


# ========================================================================================================= row kernels
@pytest.mark.parametrize("Cc", pr.ROWDOT_DIMS)
def test_rowdot(L, Cc):
    """2, 6 and 16 heads: one partial pass of 4 heads (the h < heads guard at 2 and at 6 heads) and whole passes."""
    i = pr.rowdot_inputs(Cc, pr.seed_of("rowdot", Cc))
    R, Tp = i["dO"].shape[0], i["Tp"]
    # (the inputs lie in front of spare memory of the test's own: a head pass without its guard reads past the last row)
    a, o = (torch.cat([i[k].reshape(-1), torch.zeros(1024)]).to(DEV)[:R * Cc].view(R, Cc) for k in ("dO", "O"))
    Dd = Buf((R * (Cc // 64),))
    assert L.dvt_parts_rowdot(a.data_ptr(), o.data_ptr(), Dd.ptr(), R, Tp, Cc, _s()) == 0
    torch.cuda.synchronize()
    Dd.check(f"rowdot C {Cc}")
    check_rows("rowdot", f"rowdot C {Cc}", pr.ref_rowdot, i, {"D": Dd.out})


@pytest.mark.parametrize("with_dres", [True, False])
@pytest.mark.parametrize("Cc,R", pr.LN_BWD_CASES)
def test_ln_bwd(L, Cc, R, with_dres):
    """One row, a partial second block of 32 (R = 33: one wave with one row), three blocks with a partial last wave (R = 70);
    rows with mean = rstd = 0 (as padded rows are kept) return dres unchanged; dgamma / dbeta accumulate onto known values."""
    i = pr.ln_bwd_inputs(Cc, R, pr.seed_of("ln_bwd", Cc, R))
    t = {k: dev(i[k]) for k in ("dy", "x", "mean", "rstd", "gamma", "dres")}
    dx, dg, db = Buf((R, Cc)), Buf((Cc,), fill=i["dgamma0"]), Buf((Cc,), fill=i["dbeta0"])
    rc = L.dvt_parts_ln_bwd(Cc, t["dy"].data_ptr(), t["x"].data_ptr(), t["mean"].data_ptr(), t["rstd"].data_ptr(), t["gamma"].data_ptr(),
                            t["dres"].data_ptr() if with_dres else None, dx.ptr(), dg.ptr(), db.ptr(), R, _s())
    torch.cuda.synchronize()
    assert rc == 0
    what = f"ln_bwd C {Cc} R {R} dres {int(with_dres)}"
    for b in (dx, dg, db):
        b.check(what)
    check_rows("ln_bwd", what, lambda j: pr.ref_ln_bwd(j, with_dres), i, {"dx": dx.out, "dgamma": dg.out, "dbeta": db.out})
    for r in i["zero_rows"]:
        want = i["dres"][r] if with_dres else torch.zeros(Cc)
        assert torch.equal(dx.out[r].cpu(), want), f"{what}: row {r} with mean = rstd = 0 is not dres"


def nan_padded_rows(t, T, Tp):
    """Device copy of t [batch * Tp][C] whose rows t >= T are NaN: the kernels decide by the row index and never read them."""
    d = dev(t).clone()
    d.view(-1, Tp, d.shape[1])[:, T:] = NAN
    return d


def check_ln_outputs(kernel, what, ref, i, bufs, T, Tp):
    got = {k: b.out for k, b in bufs.items() if b is not None}
    for k, b in bufs.items():
        if b is not None:
            b.check(f"{what} {k}")
            zeros_exactly(b.out.view(i["batch"], Tp, -1)[:, T:], f"{what} {k} padded rows")
    check_rows(kernel, what, ref, i, got)


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("mode", pr.ADD_LN_MODES)
@pytest.mark.parametrize("Cc", pr.DIMS)
def test_add_ln(L, Cc, mode, offset):
    """sum = a (+ b), xn = LayerNorm(sum), mean, rstd at T = 5 of Tp = 8 rows per image: packed a with pos_embed, padded a with
    padded b, b = NULL, sum_out = NULL; `offset`: rows of mean 100 and deviation 1 (the two-pass variance).  C = 384: the second
    float4 pass of a row is half idle."""
    i = pr.add_ln_inputs(Cc, pr.seed_of("add_ln", Cc, offset), offset=offset)
    T, Tp, B = i["T"], i["Tp"], i["batch"]
    R = B * Tp
    base = "pad_pad" if mode == "no_sum" else mode
    packed = base == "packed_pos"
    a = dev(i["a_packed"]) if packed else nan_padded_rows(i["a_pad"], T, Tp)
    b = dev(i["pos"]) if packed else (nan_padded_rows(i["b_pad"], T, Tp) if base == "pad_pad" else None)
    gm, be = dev(i["gamma"]), dev(i["beta"])
    bufs = {"sum": None if mode == "no_sum" else Buf((R, Cc)), "xn": Buf((R, Cc)), "mean": Buf((R,)), "rstd": Buf((R,))}
    rc = L.dvt_parts_add_ln(Cc, a.data_ptr(), int(packed), b.data_ptr() if b is not None else None, int(packed),
                            bufs["sum"].ptr() if bufs["sum"] else None, gm.data_ptr(), be.data_ptr(), bufs["xn"].ptr(), bufs["mean"].ptr(),
                            bufs["rstd"].ptr(), T, Tp, R, pr.LN_EPS, _s())
    torch.cuda.synchronize()
    assert rc == 0
    check_ln_outputs("add_ln", f"add_ln C {Cc} {mode} offset {int(offset)}", lambda j: pr.ref_add_ln(j, base), i, bufs, T, Tp)


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("mode", pr.LS_ADD_LN_MODES)
@pytest.mark.parametrize("Cc", pr.DIMS)
def test_ls_add_ln(L, Cc, mode, offset):
    """sum = a + ls (.) f, then as add_ln: with LayerScale, ls = NULL (the first block's norm1), sum_out = NULL."""
    i = pr.add_ln_inputs(Cc, pr.seed_of("add_ln", Cc, offset), offset=offset)
    T, Tp, B = i["T"], i["Tp"], i["batch"]
    R = B * Tp
    base = "ls" if mode == "no_sum" else mode
    a, f = nan_padded_rows(i["a_pad"], T, Tp), nan_padded_rows(i["f"], T, Tp)
    ls, gm, be = dev(i["ls"]), dev(i["gamma"]), dev(i["beta"])
    bufs = {"sum": None if mode == "no_sum" else Buf((R, Cc)), "xn": Buf((R, Cc)), "mean": Buf((R,)), "rstd": Buf((R,))}
    with_ls = base == "ls"
    rc = L.dvt_parts_ls_add_ln(Cc, a.data_ptr(), f.data_ptr() if with_ls else None, ls.data_ptr() if with_ls else None,
                               bufs["sum"].ptr() if bufs["sum"] else None, gm.data_ptr(), be.data_ptr(), bufs["xn"].ptr(),
                               bufs["mean"].ptr(), bufs["rstd"].ptr(), T, Tp, R, pr.LN_EPS, _s())
    torch.cuda.synchronize()
    assert rc == 0
    check_ln_outputs("ls_add_ln", f"ls_add_ln C {Cc} {mode} offset {int(offset)}", lambda j: pr.ref_add_ln(j, base), i, bufs, T, Tp)


@pytest.mark.parametrize("Cc", pr.DIMS)
def test_ls_bwd(L, Cc):
    R = 70
    i = pr.ls_bwd_inputs(Cc, R, pr.seed_of("ls_bwd", Cc))
    dy, f, ls = dev(i["dy"]), dev(i["f"]), dev(i["ls"])
    df, dls = Buf((R, Cc)), Buf((Cc,), fill=i["dls0"])
    assert L.dvt_parts_ls_bwd(Cc, dy.data_ptr(), f.data_ptr(), ls.data_ptr(), df.ptr(), dls.ptr(), R, _s()) == 0
    torch.cuda.synchronize()
    df.check("ls_bwd df")
    dls.check("ls_bwd dls")
    check_rows("ls_bwd", f"ls_bwd C {Cc}", pr.ref_ls_bwd, i, {"df": df.out, "dls": dls.out})


@pytest.mark.parametrize("backward", [0, 1])
def test_gelu(L, backward):
    """n4 = 1000 float4 (a partial last block): +-0, +-1e-4, +-1, +-8, +-30 at both ends, random values between."""
    i = pr.gelu_inputs(pr.seed_of("gelu"))
    n = i["h"].numel()
    h = dev(i["h"])
    a = Buf((n,), fill=i["da"] if backward else None)
    assert L.dvt_parts_gelu(h.data_ptr(), a.ptr(), n // 4, backward, _s()) == 0
    torch.cuda.synchronize()
    a.check("gelu")
    if backward:
        check_rows("gelu_bwd", "gelu backward", pr.ref_gelu_bwd, i, {"da": a.out})
    else:
        check_rows("gelu", "gelu forward", pr.ref_gelu, i, {"a": a.out})


@pytest.mark.parametrize("backward", [0, 1])
def test_softmax_fallback_passes(L, backward):
    """The separate softmax passes the trainer uses when tokens_pad is 64 (no whole 128-row block): Tp = 64, T = 49, 2 x 2 heads."""
    i = pr.softmax_inputs(pr.seed_of("softmax"))
    T, Tp = i["T"], i["Tp"]
    nb = i["S"].shape[0]
    S = Buf((nb, Tp, Tp), fill=i["dP"] if backward else i["S"])
    P = dev(i["P"])
    assert L.dvt_parts_softmax(P.data_ptr() if backward else None, S.ptr(), T, Tp, nb * Tp, i["scale"], backward, _s()) == 0
    torch.cuda.synchronize()
    S.check("softmax")
    zeros_exactly(S.out[:, T:], "softmax padded query rows")
    zeros_exactly(S.out[:, :, T:], "softmax padded key columns")
    if backward:
        check_rows("softmax_bwd", "softmax backward", pr.ref_softmax_bwd, i, {"dS": S.out})
    else:
        check_rows("softmax", "softmax forward", pr.ref_softmax, i, {"P": S.out})


@pytest.mark.parametrize("Cc,add,npf,nb", pr.LOSS_CASES)
def test_loss_rows(L, Cc, add, npf, nb):
    """MSE + 1 - cosine and its gradient over rows n_prefix <= t < T = 9 of Tp = 12 (the buffers are padded, the launch covers
    exactly batch * Tp rows), normalised for 2 (the whole batch) or 4 images (a slice); one all-zero target row (the 1e-8 clamp)."""
    i = pr.loss_inputs(Cc, pr.seed_of("loss", Cc, npf), npf)
    T, Tp, B = i["T"], i["Tp"], i["batch"]
    R = B * Tp

    def rows(t):  # prefix and padded rows are never read
        d = nan_padded_rows(t, T, Tp)
        d.view(B, Tp, Cc)[:, :npf] = NAN
        return d
    a, b, tg = rows(i["a"]), rows(i["b"]), dev(i["target"])
    out, dout, acc, loss = Buf((B * (T - npf), Cc)), Buf((R, Cc)), Buf((64,)), Buf((4,))
    rc = L.dvt_parts_loss_rows(Cc, a.data_ptr(), b.data_ptr() if add else None, tg.data_ptr(), out.ptr(), dout.ptr(), acc.ptr(), npf, T,
                               Tp, R, nb, loss.ptr(), add, _s())
    torch.cuda.synchronize()
    assert rc == 0
    what = f"loss_rows C {Cc} add {add} prefix {npf} norm {nb}"
    for bf in (out, dout, acc, loss):
        bf.check(what)
    d3 = dout.out.view(B, Tp, Cc)
    zeros_exactly(d3[:, :npf], what + " prefix rows of dout")
    zeros_exactly(d3[:, T:], what + " padded rows of dout")
    assert float(loss.out[3]) == 0.0
    check_rows("loss_rows", what, lambda j: pr.ref_loss(j, add, nb), i, {"dout": dout.out, "out": out.out, "loss": loss.out})


def test_pos_grad(L):
    i = pr.pos_grad_inputs(pr.seed_of("pos_grad"))
    T, Tp, B = i["T"], i["Tp"], i["batch"]
    Cc = i["dx"].shape[1]
    dx = nan_padded_rows(i["dx"], T, Tp)
    dpos = Buf((T, Cc), fill=i["dpos0"])
    assert L.dvt_parts_pos_grad(dx.data_ptr(), dpos.ptr(), B, T, Tp, Cc, _s()) == 0
    torch.cuda.synchronize()
    dpos.check("pos_grad")
    check_rows("pos_grad", "pos_grad", pr.ref_pos_grad, i, {"dpos": dpos.out})


@pytest.mark.parametrize("npf,hc", pr.EMBED_CASES)
def test_s3_embed_and_backward(L, npf, hc):
    """Token assembly of a 2 x 3 grid with 1 or 5 prefix tokens, with and without a cls row in pos_embed, s_pad = 128, batch 3;
    the backward accumulates onto known dprefix / dpos and zeroes the prefix rows of dx."""
    i = pr.embed_inputs(pr.seed_of("embed", npf, hc), npf, hc)
    B, sp, nt = i["batch"], i["s_pad"], i["n_tokens"]
    dim = i["y"].shape[1]
    y = nan_padded_rows(i["y"], nt, sp)
    y.view(B, sp, dim)[:, :npf] = NAN  # the patch embedding's prefix rows are not read either
    prefix, pos = dev(i["prefix"]), dev(i["pos"])
    x = Buf((B * sp, dim))
    assert L.dvt_parts_s3_embed(y.data_ptr(), x.ptr(), prefix.data_ptr(), pos.data_ptr(), B, dim, npf, nt, sp, hc, _s()) == 0
    torch.cuda.synchronize()
    what = f"s3_embed prefix {npf} cls {hc}"
    x.check(what)
    zeros_exactly(x.out.view(B, sp, dim)[:, nt:], what + " padded rows")
    check_rows("s3_embed", what, pr.ref_embed, i, {"x": x.out})
    dx, dpf, dps = Buf((B * sp, dim), fill=i["dx"]), Buf((npf, dim), fill=i["dprefix0"]), Buf(tuple(i["pos"].shape), fill=i["dpos0"])
    assert L.dvt_parts_s3_embed_bwd(dx.ptr(), dpf.ptr(), dps.ptr(), B, dim, npf, nt, sp, hc, _s()) == 0
    torch.cuda.synchronize()
    for bf in (dx, dpf, dps):
        bf.check(what + " backward")
    zeros_exactly(dx.out.view(B, sp, dim)[:, :npf], what + " prefix rows of dx")
    r = check_rows("s3_embed_bwd", what + " backward", pr.ref_embed_bwd, i, {"dprefix": dpf.out, "dpos": dps.out})
    assert torch.equal(dx.out.cpu().double(), r["dx"][0]), "dx: rows other than the prefix must stay bit for bit"


def test_s3_im2col(L):
    """Patch 14, stride 7, image 28 x 35 (a 3 x 4 grid of overlapping patches), k_patch 640: a copy, compared bit for bit; the
    tail columns, the 5 prefix rows and the padded rows exactly 0."""
    i = pr.im2col_inputs(pr.seed_of("im2col"))
    B, sp, kp = i["batch"], i["s_pad"], i["k_patch"]
    img = dev(i["img"])
    col = Buf((B * sp, kp))
    rc = L.dvt_parts_s3_im2col(img.data_ptr(), col.ptr(), B, i["patch"], i["stride"], i["img_h"], i["img_w"], i["grid_h"], i["grid_w"],
                               i["n_prefix"], sp, kp, _s())
    torch.cuda.synchronize()
    assert rc == 0
    col.check("im2col")
    ref = pr.ref_im2col(i)["col"][0]
    got = col.out.cpu()
    g3 = got.view(B, sp, kp)
    n = i["n_prefix"] + i["grid_h"] * i["grid_w"]
    zeros_exactly(g3[:, :i["n_prefix"]], "im2col prefix rows")
    zeros_exactly(g3[:, n:], "im2col padded rows")
    zeros_exactly(g3[:, :, 3 * i["patch"] ** 2:], "im2col tail columns")
    assert torch.equal(got, ref)
    assert L.dvt_parts_s3_im2col(img.data_ptr(), col.ptr(), B, 14, 7, 28, 34, 3, 4, 5, sp, kp, _s()) == BADARG  # grid past the image


def test_row_kernel_refusals(L):
    """Bad shapes are refused before any launch: outputs untouched."""
    t = torch.zeros(64, 1024, device=DEV)
    o = Buf((64, 1024))
    p = t.data_ptr()
    assert L.dvt_parts_ln_bwd(512, p, p, p, p, p, None, o.ptr(), o.ptr(), o.ptr(), 8, _s()) == BADARG
    assert L.dvt_parts_add_ln(384, p, 0, None, 0, None, p, p, o.ptr(), o.ptr(), o.ptr(), 9, 8, 16, 1e-6, _s()) == BADARG  # T > Tp
    assert L.dvt_parts_ls_add_ln(384, p, None, p, None, p, p, o.ptr(), o.ptr(), o.ptr(), 5, 8, 16, 1e-6, _s()) == BADARG  # ls without f
    assert L.dvt_parts_rowdot(p, p, o.ptr(), 6, 4, 128, _s()) == BADARG  # R % Tp
    assert L.dvt_parts_rowdot(p, p, o.ptr(), 6, 3, 96, _s()) == BADARG  # C % 64
    assert L.dvt_parts_gelu(p, o.ptr(), 0, 0, _s()) == BADARG
    assert L.dvt_parts_softmax(None, o.ptr(), 49, 62, 64, 0.125, 0, _s()) == BADARG  # Tp % 4
    assert L.dvt_parts_softmax(None, o.ptr(), 49, 64, 64, 0.125, 1, _s()) == BADARG  # backward without P
    assert L.dvt_parts_loss_rows(384, p, None, p, None, o.ptr(), o.ptr(), 0, 9, 12, 24, 2, o.ptr(), 1, _s()) == BADARG  # add without b
    assert L.dvt_parts_loss_rows(384, p, None, p, None, o.ptr(), o.ptr(), 9, 9, 12, 24, 2, o.ptr(), 0, _s()) == BADARG  # no loss rows
    assert L.dvt_parts_loss_rows(384, p, None, p, None, o.ptr(), o.ptr(), 0, 9, 12, 24, 1, o.ptr(), 0, _s()) == BADARG  # norm_batch < batch
    assert L.dvt_parts_pos_grad(p, o.ptr(), 2, 9, 8, 384, _s()) == BADARG
    assert L.dvt_parts_ls_bwd(100, p, p, p, o.ptr(), o.ptr(), 8, _s()) == BADARG
    assert L.dvt_parts_s3_embed(p, o.ptr(), p, p, 1, 384, 5, 5, 128, 0, _s()) == BADARG  # no patch tokens
    assert L.dvt_parts_s3_embed_bwd(o.ptr(), o.ptr(), o.ptr(), 1, 384, 1, 7, 4, 0, _s()) == BADARG  # s_pad < n_tokens
    assert L.dvt_parts_lin_fwd(p, p, None, o.ptr(), 64, 128, 96, _s()) == BADARG  # no whole k-tile, not the 128-tile's shape
    assert L.dvt_parts_lin_bwd(p, p, p, o.ptr(), o.ptr(), o.ptr(), None, 64, 96, 64, _s()) == BADARG
    torch.cuda.synchronize()
    o.untouched("refused row kernels")


def test_zz_report():
    """The worst err / tol per kernel of this run (the module docstring keeps the figures of the MI355X run)."""
    for k in sorted(RATIOS):
        print(f"worst err/tol {k}: {RATIOS[k]:.3f}")
