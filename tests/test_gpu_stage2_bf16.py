"""GPU: the opt-in bf16 modes of the stage-2 training step (include/dvt_stage2.h `dvt_s2_train_step_mp`, DESIGN section 19;
`Stage2Engine(dtype=, attention=, weight_grad=)`, `Denoiser(train_dtype=...)`).

Mode 0 through the new entry point against `dvt_s2_train_step` in bits; gemm_modes 1, 3, 5, 7 for one step against float64
autograd with the comparator of tests/s2_bf16_reference.py as the yardstick (at most 2 x the comparator's own distance, per
tensor: the bound of tests/test_gpu_stage3_bf16.py / _wgrad.py); determinism and accumulation of the split-K weight gradients;
five AdamW steps by the rule of tests/test_gpu_stage3_wgrad.py; the `Denoiser` module around a bf16 engine.

Shapes (h, w, c, blocks, batch) -> T, Tp, R:  (11, 11, 384, 1, 2) -> 121, 128, 256 the base case, also without pos_embed;
(5, 9, 384, 2, 3) -> 45, 128, 384: two blocks, R an odd multiple of 128 (the 128 x 128 bf16 GEMM tile), one weight-gradient
chunk;  (12, 12, 768, 1, 2) -> 144, 256, 512: two 128-key blocks, a masked tail tile."""
import ctypes as C
import functools

import pytest
import torch

from oracle import stage2 as O
from tests import s2_bf16_reference as S2REF
from tests.test_gpu_stage2 import DEV, _recorder, rel

pytestmark = pytest.mark.gpu

SHAPES = [(11, 11, 384, 1, 2), (5, 9, 384, 2, 3), (12, 12, 768, 1, 2)]
CASES = [s + (True,) for s in SHAPES] + [SHAPES[0] + (False,)]
MODES = (1, 3, 5, 7)
TRAIN = {0: {}, 1: dict(train_dtype="bfloat16"), 3: dict(train_dtype="bfloat16", train_attention="bfloat16"),
         5: dict(train_dtype="bfloat16", train_weight_grad="bfloat16"),
         7: dict(train_dtype="bfloat16", train_attention="bfloat16", train_weight_grad="bfloat16")}
LINEAR = ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")


@functools.lru_cache(maxsize=None)
def problem(case, seed=1):
    """(oracle model, x, target): `make_pair` of tests/test_gpu_stage2.py (perturbed LayerNorm parameters) and its batches."""
    h, w, c, blocks, batch, enable_pe = case
    torch.manual_seed(seed)
    ref = O.Denoiser(h, w, c, enable_pe, blocks)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    torch.manual_seed(seed + 1)
    return ref, torch.randn(batch, h, w, c), torch.randn(batch, h, w, c)


def model_for(case, mode, ref=None):
    from dvt_amd.models import Denoiser
    h, w, c, blocks, batch, enable_pe = case
    mine = Denoiser(h, w, c, None, enable_pe, blocks, device=DEV, **TRAIN[mode])
    assert mine.engine.gemm_mode == mode and mine.engine.cfg.tokens_pad % (128 if mode else 64) == 0
    mine.load_state_dict((ref or problem(case)[0]).state_dict())
    return mine


@functools.lru_cache(maxsize=None)
def float64_step(case):
    ref, x, t = problem(case)
    return S2REF.oracle_step(ref, x, t)


@functools.lru_cache(maxsize=None)
def comparator_step(case, mode):
    ref, x, t = problem(case)
    return S2REF.step(ref.state_dict(), x, t, mode)


@functools.lru_cache(maxsize=None)
def gpu_step(case, mode):
    """(loss, pred, gradients, gradients after a SECOND call on the same input) of a fresh model."""
    ref, x, t = problem(case)
    mine = model_for(case, mode)
    pred = torch.empty(x.shape, device=DEV)
    loss = mine.training_step(x.to(DEV), t.to(DEV), pred).cpu().clone()
    grads = {k: v.cpu().clone() for k, v in mine.engine.views(mine.engine.grads).items()}
    mine.training_step(x.to(DEV), t.to(DEV))
    twice = {k: v.cpu().clone() for k, v in mine.engine.views(mine.engine.grads).items()}
    return loss, pred.cpu(), grads, twice


# ---- mode 0 through the new entry point -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_mode0_is_the_fp32_step(case):
    """`dvt_s2_train_step_mp(..., 0)` on the engine, workspace and input of a `dvt_s2_train_step` call: weight and bias
    gradients, the pos_embed gradient and pred have the same bits; the LayerNorm gradients, which the fp32 path sums with
    float atomics, are held to the bound tools/record_s2_parent_digests.py uses for such tensors at zero recorded spread
    (8 ulp of the tensor's largest value, per element); the loss's bits are `test_mode0_loss_has_the_fp32_steps_bits`'s."""
    mode0_pair(case, check_gradients=True)


@pytest.mark.parametrize("case", CASES)
def test_mode0_loss_has_the_fp32_steps_bits(case):
    """The four loss floats of `dvt_s2_train_step_mp(..., 0)` equal those of `dvt_s2_train_step` bit for bit.  Both calls run
    the same launches; the loss kernel adds its per-workgroup sums of squared error and of cosine as 128-bit fixed-point
    integers (`loss_acc_add` in csrc/dvt_block_train.hip), which no order of arrival changes.  (With the float atomics the
    kernel used before, the two calls came out 1 .. 2 ulp apart on an MI355X in all four cases -- 3.0478343963623047 against
    3.047834634780884 in the first -- and so did two runs of `dvt_s2_train_step` itself.)"""
    loss, loss_mp = mode0_pair(case, check_gradients=False)
    bits = lambda v: v.contiguous().view(torch.int32)  # noqa: E731
    assert torch.equal(bits(loss_mp), bits(loss)), (loss_mp.tolist(), loss.tolist())


def mode0_pair(case, check_gradients):
    """One `dvt_s2_train_step`, then one `dvt_s2_train_step_mp(..., 0)` on the same engine, workspace and input -> the two
    loss tensors; with `check_gradients` everything else of the two calls is compared on the way."""
    from dvt_amd import _lib
    H = _recorder("record_s3_golden")
    _, x, t = problem(case)
    mine = model_for(case, 0)
    eng = mine.engine
    b = x.shape[0]
    xd, td = x.to(DEV).reshape(b, -1, x.shape[-1]), t.to(DEV).reshape(b, -1, x.shape[-1])
    pred = torch.empty_like(xd)
    loss = eng.train_step(xd, td, pred).cpu().clone()
    want_pred, want = pred.cpu().clone(), {k: v.cpu().clone() for k, v in eng.views(eng.grads).items()}
    L = _lib.lib()
    n = int(L.dvt_s2_workspace_bytes_mp(C.byref(eng.cfg), b, 1, 0))
    assert n == int(L.dvt_s2_workspace_bytes(C.byref(eng.cfg), b, 1))
    work = eng._workspace(b, True)
    assert work.numel() == n
    eng.grads.zero_()
    pred.fill_(float("nan"))
    loss_mp = torch.zeros(4, device=DEV)
    _lib.check(L.dvt_s2_train_step_mp(C.byref(eng.cfg), _lib.ptr(eng.params), _lib.ptr(eng.grads), _lib.ptr(xd), _lib.ptr(td),
                                      _lib.ptr(pred), b, _lib.ptr(work), work.numel(), _lib.ptr(loss_mp), _lib.stream(), 0),
               "dvt_s2_train_step_mp")
    got = {k: v.cpu().clone() for k, v in eng.views(eng.grads).items()}
    bits = lambda v: v.contiguous().view(torch.int32)  # noqa: E731
    print(f"mode 0 {case}: loss {loss.tolist()} / {loss_mp.cpu().tolist()}")
    if not check_gradients:
        return loss, loss_mp.cpu()
    assert torch.equal(bits(pred.cpu()), bits(want_pred))
    atomic = [k for k in got if H.is_atomic("grads." + k)]
    assert len(atomic) == 4 * case[3]
    moved = [k for k in got if k not in atomic and not torch.equal(bits(got[k]), bits(want[k]))]
    assert not moved, {k: rel(got[k], want[k]) for k in moved}
    for k in atomic:
        err, tol = float((got[k] - want[k]).abs().max()), H.tolerance(want[k], 0.0)
        print(f"  {k} (atomics): |difference| {err:.3e}, bound {tol:.3e}")
        assert err <= tol, (k, err, tol)
    err, tol = float((loss_mp.cpu() - loss).abs().max()), H.tolerance(loss, 0.0)
    assert err <= tol, (loss_mp.cpu().tolist(), loss.tolist())
    return loss, loss_mp.cpu()


@pytest.mark.parametrize("mode", [0, 7])
def test_loss_reproduces_its_bits_and_stays_non_finite_on_nan(mode):
    """Two steps of one engine on one input give the same four loss floats (the loss sums are integer sums); an input with one
    NaN still gives a non-finite loss, which is what the trainers' non-finite check reads."""
    case = CASES[1]
    _, x, t = problem(case)
    mine = model_for(case, mode)
    first = mine.training_step(x.to(DEV), t.to(DEV)).cpu().clone()
    again = mine.training_step(x.to(DEV), t.to(DEV)).cpu().clone()
    assert bool(torch.isfinite(first).all()) and torch.equal(first.view(torch.int32), again.view(torch.int32))
    bad = x.clone()
    bad[1, 2, 3, 5] = float("nan")
    assert not bool(torch.isfinite(mine.training_step(bad.to(DEV), t.to(DEV)).cpu()[:3]).all())


# ---- one step of every mode against float64 ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_step_vs_float64(case, mode):
    """Per gradient tensor (pos_embed's included), pred and the loss triple: relative-L2 distance from float64 autograd at most
    2 x the comparator's own; in modes 3 and 7 the k third of every qkv bias gradient is exactly zero and the other thirds
    are not.
    Measured on an MI355X, worst ratio over the four cases: mode 1 1.034 (denoiser.norm2.weight), mode 3 1.065
    (denoiser.0.attn.qkv.bias), mode 5 1.034, mode 7 1.065 (the same tensors); pred within 0.1 % of the comparator's distance."""
    f64_p, f64_l, f64_g = float64_step(case)
    cmp_p, cmp_l, cmp_g = comparator_step(case, mode)
    loss, pred, grads, _ = gpu_step(case, mode)
    assert set(grads) == set(f64_g) and (("pos_embed" in grads) == case[5])
    ratios = {}
    for k in sorted(grads):
        got, yard = rel(grads[k], f64_g[k]), rel(cmp_g[k], f64_g[k])
        ratios[k] = got / yard
        print(f"  mode {mode} {case} {k}: step {got:.3e}, comparator {yard:.3e}, ratio {ratios[k]:.3f}")
    worst = max(ratios, key=ratios.get)
    got_l, yard_l = rel(loss[:3], torch.tensor(f64_l)), rel(torch.tensor(cmp_l), torch.tensor(f64_l))
    print(f"stage-2 mode {mode} step vs float64 {case}: worst ratio {ratios[worst]:.3f} ({worst}); pred "
          f"{rel(pred, f64_p):.3e} vs comparator {rel(cmp_p, f64_p):.3e}; loss triple {got_l:.3e} vs comparator {yard_l:.3e}")
    assert bool(torch.isfinite(loss).all())
    assert rel(pred, f64_p) <= 2 * rel(cmp_p, f64_p)
    c = case[2]
    for k in grads:
        if k.endswith("attn.qkv.bias"):
            assert grads[k][:c].any() and grads[k][2 * c:].any()
            assert bool(grads[k][c:2 * c].any()) == (not mode & 2), k
    bad = {k: v for k, v in ratios.items() if not v <= 2.0}
    assert not bad, bad
    # the loss is three fp32 numbers summed over the rows with float atomics: where the rounding moves it by less than that (in
    # modes 1 and 5 the comparator's loss lies within 1e-7 of float64), the format's own bound for such sums holds instead --
    # 8 ulp, the bound of tools/record_s3_golden.py `tolerance`
    assert got_l <= max(2 * yard_l, 8 * 2.0 ** -23), (loss.tolist(), f64_l, cmp_l)


@pytest.mark.parametrize("mode", [5, 7])
@pytest.mark.parametrize("case", CASES)
def test_weight_gradients_reproduce_and_accumulate(case, mode):
    """Two fresh runs give the same bits for the four weight gradients of each block (the split-K kernel has no atomics); a
    second call on the same engine ACCUMULATES: 2 x the first, to 1e-6."""
    loss, _, grads, twice = gpu_step(case, mode)
    ref, x, t = problem(case)
    again = model_for(case, mode)
    again.training_step(x.to(DEV), t.to(DEV))
    g2 = {k: v.cpu() for k, v in again.engine.views(again.engine.grads).items()}
    weights = [k for k in grads if any(k.endswith(n + ".weight") for n in LINEAR)]
    assert len(weights) == 4 * case[3]
    bits = lambda v: v.contiguous().view(torch.int32)  # noqa: E731
    moved = [k for k in weights if not torch.equal(bits(g2[k]), bits(grads[k]))]
    assert not moved, {k: rel(g2[k], grads[k]) for k in moved}
    for k in weights:
        assert rel(twice[k], 2 * grads[k]) < 1e-6, (k, rel(twice[k], 2 * grads[k]))


# ---- a short run ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_short_run_follows_comparator_adamw(mode):
    """Five AdamW steps by the rule of tests/test_gpu_stage3_wgrad.py `test_short_run_follows_comparator_adamw` (its schedule,
    its noise on the input, its weight decay): the engine against the comparator stepped by torch.optim.AdamW; per parameter
    tensor the distance from the comparator is at most the larger of (a) 2 x the distance at which the fp32 engine follows
    float64 autograd in the same run and (b) the comparator's own distance from float64 autograd, both measured here."""
    from dvt_amd.stage2 import CosineScheduler
    case = CASES[0]
    ref, x, t = problem(case, seed=7)
    sd = ref.state_dict()
    steps, wd = 5, 1e-5
    sched = CosineScheduler(2e-4, 1e-6, steps, warmup_iters=int(0.15 * steps) or 1, start_warmup_value=0)
    p64, pmp = S2REF.leaves(sd), S2REF.leaves(sd)
    opts = [torch.optim.AdamW(list(p.values()), lr=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd) for p in (p64, pmp)]
    e32, e16 = model_for(case, 0, ref), model_for(case, mode, ref)
    gen = torch.Generator().manual_seed(11)
    for i in range(steps):
        xi = x + 0.1 * torch.randn(x.shape, generator=gen)
        lr = float(sched[i])
        for opt in opts:
            for gr in opt.param_groups:
                gr["lr"] = lr
            opt.zero_grad()
        O.loss_fn(S2REF.forward(p64, xi.double(), mode, rounding=False), t.double())[0].backward()
        O.loss_fn(S2REF.forward(pmp, xi.double(), mode), t.double())[0].backward()
        for opt in opts:
            opt.step()
        for m in (e32, e16):
            m.training_step(xi.to(DEV), t.to(DEV))
            m.engine.adamw_step(lr, wd)
    v32, v16 = e32.engine.views(), e16.engine.views()
    d32 = {k: rel(v32[k], p64[k].reshape(v32[k].shape)) for k in v32}
    dcmp = {k: rel(pmp[k], p64[k]) for k in v32}
    d16 = {k: rel(v16[k], pmp[k].reshape(v16[k].shape)) for k in v32}
    ratio = {k: d16[k] / max(2 * d32[k], dcmp[k]) for k in d16}
    print(f"stage-2 five AdamW steps, mode {mode}: fp32 engine vs float64 worst {max(d32.values()):.2e}; comparator vs float64 "
          f"worst {max(dcmp.values()):.2e}; engine vs comparator worst {max(d16.values()):.2e}; worst held/bound "
          f"{max(ratio.values()):.3f} ({max(ratio, key=ratio.get)})")
    bad = {k: (d16[k], d32[k], dcmp[k]) for k in d16 if not d16[k] <= max(2 * d32[k], dcmp[k])}
    assert not bad, bad


# ---- the module ---------------------------------------------------------------------------------------------------------
def test_denoiser_module_trains_in_bf16_and_infers_in_fp32():
    """`Denoiser(train_dtype="bfloat16", train_attention="bfloat16", train_weight_grad="bfloat16")`: `training_step` runs (a
    finite loss, gradients in the arena); `forward` afterwards is the fp32 forward -- the bits of `Stage2Engine.forward` of a
    default fp32 engine holding the same parameters -- and `state_dict()` has the reference's keys in fp32."""
    from dvt_amd import s2
    case = CASES[0]
    h, w, c, blocks, batch, enable_pe = case
    ref, x, t = problem(case)
    mine = model_for(case, 7)
    loss = mine.training_step(x.to(DEV), t.to(DEV)).cpu()
    assert bool(torch.isfinite(loss).all()) and float(mine.engine.grads.abs().max()) > 0
    mine.engine.adamw_step(1e-4, 1e-5)
    sd = mine.state_dict()
    assert list(sd) == list(ref.state_dict()) and all(v.dtype == torch.float32 for v in sd.values())
    assert all(tuple(sd[k].shape) == tuple(v.shape) for k, v in ref.state_dict().items())
    assert not torch.equal(sd["denoiser.attn.qkv.weight"].cpu(), ref.state_dict()["denoiser.attn.qkv.weight"])
    plain = s2.Stage2Engine(s2.make_config(c, h * w, blocks, enable_pe), torch.device(DEV), inference_only=True)
    assert plain.gemm_mode == 0 and plain.cfg.tokens_pad == mine.engine.cfg.tokens_pad == 128
    plain.load_named({k: v.detach() for k, v in sd.items()})
    xd = x.to(DEV)
    want = plain.forward(xd.reshape(batch, h * w, c)).reshape(batch, h, w, c)
    got = mine(xd)
    assert mine.inference_dtype == "float32" and not mine._bf16
    assert torch.equal(got, want)
    assert torch.equal(got, mine.engine.forward(xd.reshape(batch, h * w, c)).reshape(batch, h, w, c))
