"""tests/attention_reference.py without a GPU: the float64 reference against torch.softmax, every CPU restatement of a kernel's
method inside the derived tolerance on every (pattern, shape) tests/test_gpu_attention_census.py launches, and the conditions
on the inputs that make the census worth running (what one key weighs against the tolerance, what a pad key would do, where
the maximum grows)."""
import math

import pytest
import torch

from tests import attention_reference as R

SMALL = [s for s in R.BF16_SHAPES if s[0] <= 576]
BIG = [s for s in R.BF16_SHAPES if s[0] > 576]
CONDITION_SHAPES = SMALL[::5] + [s for s in SMALL if s[0] in (1, 26, 64, 65, 576)] + BIG[:1]


@pytest.mark.parametrize("shape", [R.BF16_SHAPES[1], R.BF16_SHAPES[27], R.F32_SHAPES[4]], ids=R.shape_id)
@pytest.mark.parametrize("kernel", ["log2q", "f32"])
def test_reference_is_float64_softmax_attention(kernel, shape):
    n, s_pad, heads, patterns = shape
    c = R.case(kernel, n, s_pad, heads, patterns)
    _, qref, k64, v64 = R.operands(c["inp"], kernel)
    att = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", qref, k64[:, :n]), -1)
    want = torch.einsum("bhqk,bkhd->bqhd", att, v64[:, :n])
    got = c["ref"]["out"]
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert float((c["ref"]["p"].sum(-1) - 1).abs().max()) < 1e-12


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_cpu_restatement_stays_within_the_tolerance(kernel):
    """Every comparator on every (pattern, shape) of the GPU test: the bound holds for an independent evaluation of the same
    method (other summation order, libm's exp, per-row instead of per-wave growth of the maximum)."""
    worst = {}
    for n, s_pad, heads, patterns in R.SHAPES[kernel]:
        c = R.case(kernel, n, s_pad, heads, patterns)
        got = R.emulate(kernel, c["handed"], n)
        assert bool(torch.isfinite(got[:, :n]).all()), (kernel, n, s_pad)
        for name, r in zip(patterns, R.worst_ratio(got, c, n).tolist()):
            worst[name] = max(worst.get(name, 0.0), r)
            assert r <= 1.0, (kernel, name, n, s_pad, heads, r)
    print(f"\n{kernel}: worst |restatement - float64| / tol per pattern: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_census_covers_every_column_and_key():
    for n, s_pad, heads, patterns in R.BF16_SHAPES + R.F32_SHAPES + R.X3_SHAPES:
        key = torch.arange(n)
        for h in range(heads):
            cols = R.probe_column(key, h)
            assert len(set(cols.tolist())) == min(n, 64)  # n >= 64: every element has a contributing key; below: one key each
            if n >= 128:  # consecutive tiles order their columns differently: P of one tile against V^T of another shows
                assert int(cols[0]) != int(cols[64])
        v = R.census_inputs(n, s_pad, heads, patterns)["v"]
        assert torch.equal(v.bfloat16().float(), v) and bool((v[:, n:] == R.V_PAD).all())
        assert bool(((v[:, :n] != 0).sum(-1) == 1).all())


def _removal_ratio(c, b, n, heads):
    """[heads][query][key]: |change of element (query, d(key))| / tol when `key` is taken out of the softmax."""
    p = c["ref"]["p"][b][:, :n]                                         # [H][q][k]
    out = c["ref"]["out"][b, :n].permute(1, 0, 2)                       # [H][q][64]
    tol = c["tol"][b, :n].permute(1, 0, 2)
    key = torch.arange(n)
    ratios = []
    for h in range(heads):
        col = R.probe_column(key, h)
        w = R.probe_weight(key).double()
        delta = p[h] * (w[None, :] - out[h][:, col]).abs() / (1.0 - p[h])
        ratios.append(torch.where(p[h] >= 1.0, math.inf, delta / tol[h][:, col]))  # (the only key of a row: nothing is left)
    return torch.stack(ratios)


@pytest.mark.parametrize("kernel", ["log2q", "v2"])
@pytest.mark.parametrize("shape", R.BF16_SHAPES, ids=R.shape_id)
def test_one_key_weighs_more_than_three_tolerances(kernel, shape):
    """The sensitivity the census exists for.  flat: taking ANY valid key out moves an element of EVERY row by more than 3 tol.
    random: the weights of a row spread over e^(+-3 sigma), so a row's lightest key is below its own tolerance by construction;
    there, every key moves more than 3 tol in the rows where it is heavy -- a kernel that loses key k loses it for every row."""
    n, s_pad, heads, patterns = shape
    c = R.case(kernel, n, s_pad, heads, patterns)
    flat = _removal_ratio(c, patterns.index("flat"), n, heads)
    assert float(flat.min()) > 3.0, float(flat.min())
    rnd = _removal_ratio(c, patterns.index("random"), n, heads)
    assert float(rnd.amax(1).min()) > 3.0, float(rnd.amax(1).min())


@pytest.mark.parametrize("kernel", ["log2q", "v2", "f32"])
@pytest.mark.parametrize("shape", [s for s in CONDITION_SHAPES if s[1] > s[0]], ids=R.shape_id)
def test_one_pad_key_let_in_moves_rows_by_more_than_three_tolerances(kernel, shape):
    n, s_pad, heads, patterns = shape
    c = R.case(kernel, n, s_pad, heads, patterns)
    _, qref, k64, _ = R.operands(c["inp"], kernel)
    zp = torch.einsum("bqhd,bhd->bhq", qref[:, :n], k64[:, n])          # the first pad key's logit
    z = c["ref"]["z"][:, :, :n]
    m = torch.maximum(z.amax(-1), zp)
    pp = torch.exp(zp - m) / (torch.exp(z - m[..., None]).sum(-1) + torch.exp(zp - m))
    out, tol = c["ref"]["out"][:, :n].permute(0, 2, 1, 3), c["tol"][:, :n].permute(0, 2, 1, 3)
    moved = ((pp[..., None] * (R.V_PAD - out)).abs() / tol).amax(-1) > 3.0   # [B][H][q]
    assert bool(moved.any(-1).all()), "a pad key that no row of some (pattern, head) would notice"
    assert bool(moved[patterns.index("flat")].all())
    for name in ("massive+", "massive-"):
        if name in patterns:
            assert bool(moved[patterns.index(name)].all()), name


@pytest.mark.parametrize("kernel", ["log2q", "v2"])
@pytest.mark.parametrize("shape", [s for s in SMALL if s[0] > 64][::3], ids=R.shape_id)
def test_stairs_maximum_grows_past_the_vote_on_every_tile(kernel, shape):
    n, s_pad, heads, patterns = shape
    z = R.case(kernel, n, s_pad, heads, patterns)["ref"]["z"][patterns.index("stairs")][:, :n]   # [H][q][k]
    tmax = torch.stack([z[..., t0:t0 + 64].amax(-1) for t0 in range(0, n, 64)], -1)
    step = tmax[..., 1:] - tmax[..., :-1]
    assert float(step[:, 1::2].min()) > 8.0 and float(step[:, 0::2].max()) < -8.0


@pytest.mark.parametrize("kernel", ["log2q", "v2", "x3"])
@pytest.mark.parametrize("shape", [s for s in SMALL if s[0] > 64][::3] + BIG[:1], ids=R.shape_id)
def test_spikes_dominate_and_rise_on_the_intended_side_of_the_vote(kernel, shape):
    n, s_pad, heads, patterns = shape
    c = R.case(kernel, n, s_pad, heads, patterns)
    sp = R.spike_keys(n)
    i = torch.arange(n)
    for name in patterns:
        if not name.startswith("spikes"):
            continue
        b = patterns.index(name)
        z, p = c["ref"]["z"][b][:, :n], c["ref"]["p"][b][:, :n]
        every = i % 4 == 1
        for s_idx, (tile, key) in enumerate(sp):
            alone = (i % 4 == 3) & ((i // 4) % len(sp) == s_idx)
            if bool(alone.any()):
                assert float(p[:, alone, key].min()) > 0.5, (name, tile, key)
            if tile == 0:
                continue  # (tile 0's maximum is exact in every kernel: no vote)
            for rows in (alone, every):
                if not bool(rows.any()):
                    continue
                rise = z[:, rows, key] - z[:, rows, :64 * tile].amax(-1)
                big = torch.exp(rise)
                if name == "spikes8.5":
                    assert float(big.min()) > 2980.0, (tile, key, float(rise.min()))
                else:  # the lane's 16-term row sum stays below the vote: P is formed against the old maximum
                    assert float(big.max()) + 16.0 < 2980.0 and float(rise.min()) > 7.0, (tile, key, float(rise.max()))
        assert float(p[:, every, sp[-1][1]].min()) > 0.5  # the last of the rising spikes ends on top
    tiles = {t for t, _ in sp}
    nt = -(-n // 64)
    assert {nt - 1, nt - 2} <= tiles and {t % 4 for t in tiles if t >= 1} == ({0, 1, 2, 3} if nt >= 5 else {t % 4 for t in range(1, nt)})
    assert all(k < n for _, k in sp)


def test_spike_offsets_cover_the_lane_groups_and_both_halves():
    assert {(o % 16) // 4 for o in R.SPIKE_OFFSETS} == {0, 1, 2, 3} and {o // 32 for o in R.SPIKE_OFFSETS} == {0, 1}
    assert R.spike_keys(1370)[-1] == (21, 21 * 64 + 22) and 1370 - 21 * 64 <= 32   # a half tail tile carries a spike


@pytest.mark.parametrize("kernel", ["log2q", "v2", "f32"])
def test_logits_stay_inside_the_exp2_range_and_massive_is_massive(kernel):
    for n, s_pad, heads, patterns in R.SHAPES[kernel][::3] + R.SHAPES[kernel][-1:]:
        c = R.case(kernel, n, s_pad, heads, patterns)
        _, qref, k64, _ = R.operands(c["inp"], kernel)
        zall = torch.einsum("bqhd,bkhd->bhqk", qref, k64)               # pad keys and pad queries too: the MFMA forms them
        assert float(zall.abs().max()) * R.LOG2E < 126.0, (n, float(zall.abs().max()))
        for name, sign in (("massive+", 1.0), ("massive-", -1.0)):
            if name in patterns:
                z = c["ref"]["z"][patterns.index(name)][:, :n]
                assert float((sign * z).min()) > 30.0 and abs(float((sign * z).mean()) - 60.0) < 5.0


def test_launches_exercise_the_xcd_remap():
    odd = [s for s in R.BF16_SHAPES if R.workgroups(*s) > 8 and R.workgroups(*s) % 8]
    assert len(odd) >= 2
    idle = {s[1] % 128 for s in R.BF16_SHAPES}
    assert {32, 64, 96, 0} <= idle and any(s[1] < 128 for s in R.BF16_SHAPES)
    for t in range(9):  # every unroll phase twice, half and whole tails
        assert {s[0] - 64 * t for s in R.BF16_SHAPES if 64 * t < s[0] <= 64 * t + 64} >= {1, 26, 32, 33, 63, 64}
    assert math.isclose(R.FLOOR, 2.0 ** -100)
