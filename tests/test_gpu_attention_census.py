"""The attention kernels held to float64 per key (tests/attention_reference.py): V is a probe with one non-zero column per key,
so every output element is the summed probability of the one to 22 keys that map to it, and is compared with a RELATIVE bound
derived from the kernel's rounding points -- a key that is dropped, doubled, let in from the padding or met with another
tile's V^T moves an element by many tolerances where the dense-V tests of tests/test_gpu_vit.py move by 1 / n_valid.

One launch per (kernel, shape); batch = the logit patterns (flat, random, stairs, spikes at a rise of 7.5 and of 8.5, massive+,
massive-), heads 2 or 3.  Every element of every valid query row is compared; pad query rows must be finite; NaN lies in the
128 slack rows behind the last image of qk / qkv and in a spare image behind vt; the sentinel behind the last image of the output
must survive.  Shapes: attention_reference.BF16_SHAPES / F32_SHAPES / X3_SHAPES (every tile-loop phase twice, half and whole
tail tiles, idle waves at s_pad % 128 of 32 / 64 / 96, s_pad < 128, 1370 keys at a pitch of 1376 and 1408).

Measured on one MI355X, worst |got - float64| / tol over all shapes (bound 1; profiles/attention_census/README.md has the CPU
restatements' figures beside them and the break checks):
                 flat   random  stairs  spikes7.5  spikes8.5  massive+  massive-
  log2q          0.488  0.888   0.919   0.879      0.897      0.631     0.639
  v2             0.488  0.928   0.942   0.926      0.906      0.748     0.751
  f32            0.003  0.005   0.018   0.008      0.009      0.016     0.016
  x3             0.001  0.016   0.024   0.016      0.018      0.011     0.011
  x3_presplit    0.045  0.016   0.026   0.018      0.019      0.012     0.011
GPU time of the whole file: 6.0 s for its 192 cases (0.4 s the first launch of the process, 0.12 to 0.19 s a 1370-key case,
0.06 s or less every other).
"""
import pytest
import torch

from tests import attention_reference as R
from tests import test_gpu_vit as V
from tests.test_gpu_vit import DEV, _s

pytestmark = pytest.mark.gpu
SENTINEL = 7.0


@pytest.fixture(scope="module")
def L(built_lib):
    import dvt_amd.vit  # noqa: F401 registers signatures
    return built_lib


def family(variant):
    """The reference / tolerance a kernel is held to: `variant` is an entry of test_gpu_vit.ATTN_CASES / LAB_ATTN_CASES
    ("log2q", ("log2q", mask), (kernel, mask)) or "f32" / "x3"."""
    if variant in ("f32", "x3"):
        return variant
    return "log2q" if variant == "log2q" or variant[0] == "log2q" else "v2"


def _compare(got, c, n, patterns, what):
    """Every element of every valid row against its tolerance; returns the worst ratio per pattern."""
    ref, tol = c["ref"]["out"], c["tol"]
    bad = ~((got - ref).abs() <= tol)[:, :n]   # (NaN compares false: counted)
    ratios = R.worst_ratio(got, c, n).tolist()
    print(f"census {what}: " + ", ".join(f"{p} {r:.3f}" for p, r in zip(patterns, ratios)))
    if bool(bad.any()):
        b, q, h, d = (int(x) for x in bad.nonzero()[0])
        worst = ((got - ref).abs() / tol)[:, :n].nan_to_num(nan=float("inf"))
        wb, wq, wh, wd = (int(x) for x in (worst == worst.max()).nonzero()[0])
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond tol; per pattern "
            f"{dict(zip(patterns, bad.sum(dim=(1, 2, 3)).tolist()))}; first [{patterns[b]}, q {q}, h {h}, d {d}] got "
            f"{float(got[b, q, h, d]):.6g} want {float(ref[b, q, h, d]):.6g}; worst [{patterns[wb]}, q {wq}, h {wh}, d {wd}] "
            f"{float(worst.max()):.3g} tol")
    return dict(zip(patterns, ratios))


def check_attention_census(L, variant, shape):
    """One launch of one attention kernel on the census inputs of `shape` = (n_valid, s_pad, heads, patterns); for "x3" the
    presplit entry point (split_out = 1, hi + lo) on the same scratch as well.  Returns {kernel family: {pattern: worst ratio}}."""
    n, s_pad, heads, patterns = shape
    fam = family(variant)
    c = R.case(fam, n, s_pad, heads, patterns)
    qh, kh, vh = c["handed"]
    B, dim = len(patterns), heads * 64
    rows = B * s_pad
    what = f"{variant} {R.shape_id(shape)}"
    if fam in ("log2q", "v2"):
        qk = torch.full((rows + 128, 2 * dim), float("nan"), dtype=torch.bfloat16)
        qk[:rows] = torch.cat([qh.reshape(rows, dim), kh.reshape(rows, dim)], 1)
        vt = torch.full((B + 1, heads, 64, s_pad), float("nan"), dtype=torch.bfloat16)
        vt[:B] = vh.permute(0, 2, 3, 1)
        qk, vt = qk.to(DEV), vt.to(DEV)
        out = torch.full((rows + 128, dim), SENTINEL, device=DEV, dtype=torch.bfloat16)
        assert V.run_attention(L, variant, qk, vt, out, B, heads, s_pad, n) == 0
        torch.cuda.synchronize()
        outs = {fam: out}
    else:
        qkv = torch.full((rows + 128, 3 * dim), float("nan"))
        qkv[:rows] = torch.cat([qh.reshape(rows, dim), kh.reshape(rows, dim), vh.reshape(rows, dim)], 1)
        qkv = qkv.to(DEV)
        out = torch.full((rows + 128, dim), SENTINEL, device=DEV, dtype=torch.float32)
        if fam == "f32":
            assert L.dvt_vit_attention_f32(qkv.data_ptr(), out.data_ptr(), B, heads, s_pad, n, _s()) == 0
            torch.cuda.synchronize()
            outs = {fam: out}
        else:
            scratch = torch.zeros(int(L.dvt_vit_attention_x3_scratch_bytes(B, heads, s_pad)), device=DEV, dtype=torch.uint8)
            out3 = torch.full((rows + 128, 3 * dim), SENTINEL, device=DEV, dtype=torch.bfloat16)
            assert L.dvt_vit_attention_x3(qkv.data_ptr(), out.data_ptr(), scratch.data_ptr(), B, heads, s_pad, n, _s()) == 0
            assert L.dvt_vit_attention_x3_presplit(scratch.data_ptr(), out3.data_ptr(), B, heads, s_pad, n, 1, _s()) == 0
            torch.cuda.synchronize()
            assert bool((out3[rows:].float() == SENTINEL).all()), f"{what}: the split output was stored behind the last image"
            o3 = out3[:rows].cpu()
            assert torch.equal(o3[:, :dim].view(torch.int16), o3[:, dim:2 * dim].view(torch.int16)), "[hi | hi | lo]: the two hi differ"
            split = torch.zeros(rows + 128, dim, dtype=torch.float64)
            split[:rows] = o3[:, :dim].double() + o3[:, 2 * dim:].double()
            outs = {"x3": out, "x3_presplit": split}
    result = {}
    for name, o in outs.items():
        if name != "x3_presplit":
            assert bool((o[rows:].float() == SENTINEL).all()), f"{what}: a query block behind the last image stored its rows"
        got = o[:rows].double().cpu().reshape(B, s_pad, heads, 64)
        assert bool(torch.isfinite(got).all()), f"{what} ({name}): a pad query row is not finite"
        cc = c if name == fam else R.case(name, n, s_pad, heads, patterns)
        result[name] = _compare(got, cc, n, patterns, f"{what} ({name})")
    return result


@pytest.mark.parametrize("variant", V.ATTN_CASES, ids=lambda v: family(v))
@pytest.mark.parametrize("shape", R.BF16_SHAPES, ids=R.shape_id)
def test_bf16_attention_census(L, variant, shape):
    check_attention_census(L, variant, shape)


@pytest.mark.parametrize("shape", R.F32_SHAPES, ids=R.shape_id)
def test_f32_attention_census(L, shape):
    check_attention_census(L, "f32", shape)


@pytest.mark.parametrize("shape", R.X3_SHAPES, ids=R.shape_id)
def test_bf16x3_attention_census(L, shape):
    """dvt_vit_attention_x3 (fp32 rows) and dvt_vit_attention_x3_presplit(split_out = 1) (hi + lo of the [hi | hi | lo] rows)."""
    check_attention_census(L, "x3", shape)
