"""GPU: the bf16 split-K weight gradient of the stage-3 step (csrc/dvt_s3_wgrad.hip; include/dvt_stage3.h gemm_modes 5 and 7,
`Stage3Engine(dtype="bfloat16", weight_grad="bfloat16")`, `python -m dvt_amd.stage3 --weight_grad bfloat16`).

Kernel level, through `s3.wgrad_bf16`: indexing bit for bit on integer data, arithmetic against float64 within the worst case of
any fp32 summation order, accumulation, determinism.  Step level, at the shapes of tests/test_gpu_stage3_bf16.py for both modes:
one step against float64 autograd with the comparator of tests/s3_wgrad_reference.py as the yardstick (at most 2 x the
comparator's own distance, per tensor), proof that the mode is engaged and touches nothing else, slices, a short AdamW run, the
driver, and mode 3 held to the bits of the commit before the mode existed."""
import functools
import json
import math
import os

import pytest
import torch

from tests import s3_reference as REF
from tests import s3_wgrad_reference as WG
from tests.test_gpu_stage3_bf16 import DEV, ROOT, SHAPES, _image_folder, _recorder, engine_for, problem, rel

pytestmark = pytest.mark.gpu

# (R, n, k, splits): one tile and one step pair; one forced chunk over several tiles; 22 row steps in 3 uneven chunks (8, 7, 7)
# and under the rule (5 chunks: 5, 5, 4, 4, 4); qkv, fc2 and fc1 at dim 384
KERNEL_SHAPES = [(128, 128, 128, 0), (384, 384, 128, 1), (1408, 128, 384, 3), (1408, 128, 384, 0), (640, 1152, 384, 0),
                 (256, 384, 1536, 2), (256, 1536, 384, 0)]
EPS = 2.0 ** -24
ENGINE = {5: dict(dtype="bfloat16", weight_grad="bfloat16"),
          7: dict(dtype="bfloat16", attention="bfloat16", weight_grad="bfloat16"),
          1: dict(dtype="bfloat16"), 3: dict(dtype="bfloat16", attention="bfloat16")}


def bf16_64(t):
    return t.to(torch.bfloat16).double()


def run_kernel(dy, x, splits, dw=None, db=None):
    from dvt_amd import s3
    dw, db = s3.wgrad_bf16(dy.to(DEV), x.to(DEV), None if dw is None else dw.to(DEV), None if db is None else db.to(DEV), splits)
    torch.cuda.synchronize()
    return dw.cpu(), db.cpu()


# ---- kernel level ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,n,k,splits", KERNEL_SHAPES)
def test_kernel_indexing_bit_for_bit(R, n, k, splits):
    """dy[r][j] = 1 where j == r % n: dW[j] is the sum of the rows r == j (mod n) of x, db[j] their count.  x holds small
    integers (asymmetric in r and k), exact in bf16 and in any fp32 summation: every element must be exact, so a dropped,
    duplicated or misplaced row or column at any tile or chunk edge shows."""
    r = torch.arange(R)
    dy = torch.zeros(R, n)
    dy[r, r % n] = 1.0
    x = ((r[:, None] * 7 + torch.arange(k)[None, :] * 3 + (r[:, None] // 64)) % 61 - 30).float()
    want_w = torch.zeros(n, k, dtype=torch.float64).index_add_(0, r % n, x.double())
    want_b = torch.bincount(r % n, minlength=n).double()
    dw, db = run_kernel(dy, x, splits)
    assert torch.equal(dw.double(), want_w), (dw.double() - want_w).abs().max()
    assert torch.equal(db.double(), want_b)


def operands(R, n, k, spikes, seed=0):
    g = torch.Generator().manual_seed(seed + R + n + k)
    dy, x = torch.randn(R, n, generator=g), torch.randn(R, k, generator=g)
    if spikes:  # a few entries x 2^8 in both operands, some meeting in one product row
        for t, cols in ((dy, n), (x, k)):
            rows = torch.randint(0, R, (12,), generator=g)
            t[rows, torch.randint(0, cols, (12,), generator=g)] *= 256.0
        dy[5, 3] *= 256.0
        x[5, 7] *= 256.0
    return dy, x


@pytest.mark.parametrize("spikes", [False, True])
@pytest.mark.parametrize("R,n,k,splits", KERNEL_SHAPES)
def test_kernel_arithmetic_vs_float64(R, n, k, splits, spikes):
    """Per element |dW - ref| <= R 2^-24 sum_r |bf16 dy| |bf16 x| with ref the float64 product of the ROUNDED operands (products of
    two bf16 values are exact in fp32, so this is the worst case of any fp32 summation order), |db - sum dy| <= R 2^-24 sum |dy|
    against float64 of the unrounded dy, and the distance to the float64 product of the UNROUNDED operands is at least 10 x the
    distance to ref: the rounding is engaged, this is no fp32 product.
    Measured on an MI355X: worst err / bound 0.034, distance to ref 2.7e-8 .. 1.6e-7, to the unrounded product 1.4e-3 .. 2.9e-3."""
    dy, x = operands(R, n, k, spikes)
    dyb, xb = bf16_64(dy), bf16_64(x)
    ref, bound = dyb.t() @ xb, R * EPS * (dyb.abs().t() @ xb.abs())
    dw, db = run_kernel(dy, x, splits)
    err = (dw.double() - ref).abs()
    d_ref, d_exact = rel(dw, ref), rel(dw, dy.double().t() @ x.double())
    print(f"wgrad {(R, n, k, splits)} spikes={spikes}: worst err/bound {float((err / bound).max()):.3e}, rel to rounded ref "
          f"{d_ref:.3e}, rel to unrounded product {d_exact:.3e}")
    assert bool((err <= bound).all()), float((err / bound).max())
    eb = (db.double() - dy.double().sum(0)).abs()
    assert bool((eb <= R * EPS * dy.double().abs().sum(0)).all())
    assert d_exact >= 10 * d_ref, (d_exact, d_ref)


@pytest.mark.parametrize("R,n,k,splits", [(1408, 128, 384, 0), (256, 384, 1536, 2)])
def test_kernel_accumulates(R, n, k, splits):
    """accumulate = 1 onto a prefilled dw / db: the prefill plus the accumulate = 0 result, one fp32 rounding per element."""
    dy, x = operands(R, n, k, False, seed=1)
    g = torch.Generator().manual_seed(9)
    pw, pb = torch.randn(n, k, generator=g) * 30, torch.randn(n, generator=g) * 30
    dw0, db0 = run_kernel(dy, x, splits)
    dw1, db1 = run_kernel(dy, x, splits, pw.clone(), pb.clone())
    for got, pre, inc in ((dw1, pw, dw0), (db1, pb, db0)):
        want = pre.double() + inc.double()
        assert bool(((got.double() - want).abs() <= EPS * want.abs() * (1 + 1e-9)).all())  # half an ulp of the sum
        assert not torch.equal(got, inc)


def test_kernel_is_deterministic_and_splits_agree():
    """A second run gives the same bits; forced split counts give the same values within the arithmetic bound."""
    R, n, k = 1408, 128, 384
    dy, x = operands(R, n, k, True, seed=2)
    dyb, xb = bf16_64(dy), bf16_64(x)
    ref, bound = dyb.t() @ xb, R * EPS * (dyb.abs().t() @ xb.abs())
    first = run_kernel(dy, x, 0)
    again = run_kernel(dy, x, 0)
    assert torch.equal(first[0].view(torch.int32), again[0].view(torch.int32))
    assert torch.equal(first[1].view(torch.int32), again[1].view(torch.int32))
    for s in (1, 2, 3, 7, 22, 100):
        dw, db = run_kernel(dy, x, s)
        assert bool(((dw.double() - ref).abs() <= bound).all()), s
        assert torch.equal(db.view(torch.int32), first[1].view(torch.int32)), s  # (the column sum does not depend on S)


# ---- step level -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def references(shape, mode):
    """(float64 autograd, the mode's comparator) of one step at `shape`, each (features, loss triple, gradients)."""
    dim, depth, img, batch, n_reg = shape
    sd, x, t = problem(dim, depth, img, batch, n_reg)
    return REF.step(sd, x, t), WG.step(sd, x, t, attention=mode == 7)


@functools.lru_cache(maxsize=None)
def gpu_step(shape, mode):
    dim, depth, img, batch, n_reg = shape
    sd, x, t = problem(dim, depth, img, batch, n_reg)
    eng = engine_for(sd, dim, depth, img, n_reg, **ENGINE[mode])
    assert eng.gemm_mode == mode
    feat = torch.empty(t.shape, device=DEV)
    loss = eng.train_step(x.to(DEV), t.to(DEV), feat).cpu().clone()
    return loss, feat.cpu(), {k: v.cpu().clone() for k, v in eng.views(eng.grads).items()}


@pytest.mark.parametrize("mode", [5, 7])
@pytest.mark.parametrize("shape", SHAPES)
def test_step_gradients_vs_float64(shape, mode):
    """Per parameter tensor, the features and the loss triple: relative-L2 distance from float64 autograd <= 2 x the
    comparator's; in mode 7 the k third of every qkv bias gradient is exactly zero.
    Measured on an MI355X, worst ratio per shape: mode 5 1.034 (blocks.0.norm2.bias), 1.038 (norm.weight), 1.031 (cls_token);
    mode 7 1.072 (cls_token), 1.047 (blocks.0.ls2.gamma), 1.027 (blocks.0.attn.qkv.bias)."""
    (f64_f, f64_l, f64_g), (cmp_f, cmp_l, cmp_g) = references(shape, mode)
    loss, feat, grads = gpu_step(shape, mode)
    assert set(grads) == set(f64_g)
    ratios = {}
    for k in sorted(grads):
        got, yard = rel(grads[k], f64_g[k]), rel(cmp_g[k], f64_g[k])
        ratios[k] = got / yard
        print(f"  mode {mode} {shape} {k}: step {got:.3e}, comparator {yard:.3e}, ratio {ratios[k]:.3f}")
    worst = max(ratios, key=ratios.get)
    got_l, yard_l = rel(loss[:3], torch.tensor(f64_l)), rel(torch.tensor(cmp_l), torch.tensor(f64_l))
    print(f"stage-3 mode {mode} step vs float64 {shape}: worst ratio {ratios[worst]:.3f} ({worst}); features "
          f"{rel(feat, f64_f):.3e} vs comparator {rel(cmp_f, f64_f):.3e}; loss triple {got_l:.3e} vs comparator {yard_l:.3e}")
    assert rel(feat, f64_f) <= 2 * rel(cmp_f, f64_f)
    if mode == 7:
        dim = shape[0]
        assert all(not grads[k][dim:2 * dim].any() and grads[k][:dim].any() and grads[k][2 * dim:].any()
                   for k in grads if k.endswith("attn.qkv.bias"))
    bad = {k: v for k, v in ratios.items() if not v <= 2.0}
    assert not bad, bad
    assert got_l <= 2 * yard_l, (loss.tolist(), f64_l, cmp_l)


@pytest.mark.parametrize("mode", [5, 7])
def test_mode_is_engaged_and_touches_nothing_else(mode):
    """Block 0's four weight gradients differ in bits from mode 1's resp. 3's on the same input.  The other gradients of the LAST
    block and of the final norm depend on no weight gradient and are formed from the same inputs by the same arithmetic: the
    four bias gradients must have the SAME BITS as there (the column sum of csrc/dvt_s3_wgrad.hip keeps the fp32 kernel's
    order).  The LayerNorm and LayerScale gradients are summed over the rows with float atomics (`is_atomic` of
    tools/record_s3_golden.py) and do not reproduce their own bits between two runs of ONE mode -- on an MI355X ls2.gamma,
    norm.weight and norm.bias came out 4e-8 to 5e-8 relative apart between modes 1 and 5 while the other five agreed in bits --
    so they are held to that recorder's bound for such tensors at zero recorded spread: 8 ulp of the tensor's largest value,
    per element."""
    H = _recorder("record_s3_golden")
    shape = SHAPES[0]
    depth = shape[1]
    got, base = gpu_step(shape, mode)[2], gpu_step(shape, mode - 4)[2]
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    weights = [f"blocks.0.{n}.weight" for n in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")]
    same = [k for k in weights if torch.equal(bits(got[k]), bits(base[k]))]
    assert not same, same
    for k in weights:
        print(f"  mode {mode} vs mode {mode - 4}, {k}: {rel(got[k], base[k]):.3e}")
    last = f"blocks.{depth - 1}."
    lin_w = {last + n + ".weight" for n in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")}
    keep = [k for k in got if k.startswith(last) and k not in lin_w] + ["norm.weight", "norm.bias"]
    atomic = [k for k in keep if H.is_atomic("grads." + k)]
    exact = [k for k in keep if k not in atomic]
    assert sorted(exact) == sorted(last + n + ".bias" for n in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")) and len(atomic) == 8
    moved = [k for k in exact if not torch.equal(bits(got[k]), bits(base[k]))]
    assert not moved, {k: rel(got[k], base[k]) for k in moved}
    for k in atomic:
        err, tol = float((got[k] - base[k]).abs().max()), H.tolerance(base[k], 0.0)
        print(f"  mode {mode} vs mode {mode - 4}, {k} (atomics): |difference| {err:.3e}, bound {tol:.3e}")
        assert err <= tol, (k, err, tol)


@pytest.mark.parametrize("mode", [5, 7])
def test_slices_equal_whole_batch(mode):
    """Batch 4 at once and as 2 + 2 normalised by 4: the bar of tests/test_gpu_stage3_bf16.py, 1e-5.  Measured on an MI355X:
    loss 1.5e-8 / 8.9e-8, worst gradient 1.6e-7 / 1.5e-7 (modes 5 / 7)."""
    sd, x, t = problem(384, 2, 98, 4, seed=5)
    whole = engine_for(sd, 384, 2, 98, **ENGINE[mode])
    lw = whole.train_step(x.to(DEV), t.to(DEV)).cpu()
    sliced = engine_for(sd, 384, 2, 98, **ENGINE[mode])
    ls = sliced.train_step(x.to(DEV), t.to(DEV), micro_batch=2).cpu()
    gw, gs = whole.views(whole.grads), sliced.views(sliced.grads)
    errs = {k: rel(gs[k], gw[k]) for k in gw}
    print(f"stage-3 mode {mode} slices vs whole batch: loss {rel(ls[:3], lw[:3]):.2e}, worst gradient {max(errs.values()):.2e}")
    assert rel(ls[:3], lw[:3]) < 1e-5
    assert all(v < 1e-5 for v in errs.values()), errs


@pytest.mark.parametrize("mode", [5, 7])
def test_short_run_follows_comparator_adamw(mode):
    """Five AdamW steps (schedule and inputs of tests/test_gpu_stage3_bf16.py `test_short_run_follows_comparator_adamw`) of the
    engine against the comparator stepped by torch.optim.AdamW; per parameter tensor the distance from the comparator is at most
    the larger of (a) 2 x the distance at which the fp32 engine follows float64 autograd in the same run and (b) the comparator's
    own distance from float64 autograd, both measured here.
    Measured on an MI355X (worst tensor each), mode 5 / mode 7: fp32 engine against float64 3.4e-5 / 3.3e-5, comparator against
    float64 4.2e-4 / 5.0e-4, engine against the comparator 1.07e-4 / 1.95e-4, largest held / bound 0.57 (blocks.1.attn.qkv.bias) /
    0.67 (norm.weight)."""
    from dvt_amd.stage2 import CosineScheduler
    from oracle import vit as OV
    sd, x, t = problem(384, 2, 98, 2, seed=7)
    steps, wd = 5, 1e-5
    sched = CosineScheduler(2e-4, 1e-6, steps, warmup_iters=int(0.15 * steps) or 1, start_warmup_value=0)
    p64, pmp = REF.leaves(sd), REF.leaves(sd)
    opts = [torch.optim.AdamW(list(p.values()), lr=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd) for p in (p64, pmp)]
    e32, e16 = engine_for(sd, 384, 2, 98), engine_for(sd, 384, 2, 98, **ENGINE[mode])
    gen = torch.Generator().manual_seed(11)
    for i in range(steps):
        xi = x + 0.1 * torch.randn(x.shape, generator=gen)
        lr = float(sched[i])
        for opt in opts:
            for gr in opt.param_groups:
                gr["lr"] = lr
            opt.zero_grad()
        REF.loss_fn(OV.forward_features(p64, xi.double(), patch=14, stride=14), t.double())[0].backward()
        REF.loss_fn(WG.forward_features(pmp, xi.double(), 14, 14, attention=mode == 7), t.double())[0].backward()
        for opt in opts:
            opt.step()
        for eng in (e32, e16):
            eng.train_step(xi.to(DEV), t.to(DEV))
            eng.adamw_step(lr, wd)
    v32, v16 = e32.views(), e16.views()
    d32 = {k: rel(v32[k], p64[k]) for k in v32}
    dcmp = {k: rel(pmp[k], p64[k]) for k in v32}
    d16 = {k: rel(v16[k], pmp[k]) for k in v32}
    ratio = {k: d16[k] / max(2 * d32[k], dcmp[k]) for k in d16}
    print(f"stage-3 five AdamW steps, mode {mode}: fp32 engine vs float64 worst {max(d32.values()):.2e}; comparator vs float64 "
          f"worst {max(dcmp.values()):.2e}; engine vs comparator worst {max(d16.values()):.2e}; worst held/bound "
          f"{max(ratio.values()):.3f} ({max(ratio, key=ratio.get)})")
    bad = {k: (d16[k], d32[k], dcmp[k]) for k in d16 if not d16[k] <= max(2 * d32[k], dcmp[k])}
    assert not bad, bad


def test_driver_bf16_weight_grad(tmp_path, capsys):
    """`stage3.main --dtype bfloat16 --attention bfloat16 --weight_grad bfloat16` for two steps on the tiny image folder: the
    banner names the weight gradients, the losses are finite, the checkpoint is fp32, trained, and the wrapper loads it."""
    from dvt_amd import stage2, stage3
    from dvt_amd.models import Denoiser
    from dvt_amd.vit import random_state_dict
    root = str(tmp_path)
    _image_folder(f"{root}/images")
    sd = random_state_dict(384, 12, 14, 1 + 49, seed=4, well_conditioned=True)
    torch.save(sd, f"{root}/vit_s.pth")
    den = Denoiser(7, 7, 384, None, num_blocks=1, device=DEV, seed=0)
    os.makedirs(f"{root}/s2/checkpoints")
    stage2.save_checkpoint(f"{root}/s2", den, 0, 1e-4, 1e-5)
    del den
    args = ["--model", "vit_small_patch14_dinov2.lvd142m", "--denoiser_ckpt", f"{root}/s2/checkpoints/ckpt_000000.pth",
            "--data_root", f"{root}/images", "--input_size", "98", "98", "--auto_stride", "--batch_size", "2",
            "--num_iterations", "2", "--save_freq", "1", "--log_freq", "1", "--num_workers", "2", "--output_root",
            f"{root}/work", "--vit_checkpoint", f"{root}/vit_s.pth"]
    with pytest.raises(SystemExit, match="--weight_grad bfloat16 needs --dtype bfloat16"):
        stage3.main(args + ["--weight_grad", "bfloat16"])
    assert not os.path.exists(f"{root}/work")
    stage3.main(args + ["--dtype", "bfloat16", "--attention", "bfloat16", "--weight_grad", "bfloat16"])
    out = capsys.readouterr().out
    assert "student weight gradients bfloat16" in out and "student attention bfloat16" in out
    losses = [float(line.split("loss:")[1].split()[0]) for line in out.splitlines() if line.startswith("Train ")]
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses), out
    path = f"{root}/work/denosing-vit/debug/checkpoints/latest.pth"
    ck = torch.load(path, weights_only=False)
    assert set(ck) == {"model", "optimizer", "step"} and set(ck["model"]) == {"model." + k for k in sd}
    assert all(v.dtype == torch.float32 for v in ck["model"].values())
    assert not torch.equal(ck["model"]["model.blocks.0.attn.qkv.weight"], sd["blocks.0.attn.qkv.weight"])
    from dvt_amd.models.vit_wrapper import PretrainedViTWrapper
    w = PretrainedViTWrapper("vit_small_patch14_dinov2.lvd142m", stride=14, checkpoint_path=path, img_size=(98, 98),
                             dtype="float32")
    assert all(torch.equal(w._state_dict[k], ck["model"]["model." + k]) for k in sd)


# ---- mode 3 keeps the bits of the commit before modes 5 and 7 existed ------------------------------------------------
def test_bf16_attention_path_keeps_the_parents_bits(golden_dir):
    """`carve` and `run` of csrc/dvt_stage3.hip now test gemm_mode bit by bit, and the block's weight-gradient call grew a branch:
    one gemm_mode 3 step at the first shape against what `tools/record_s3_parent_digests.py --bf16 --attention` recorded from the
    commit before that (tests/golden/s3_bf16_attn_parent_digests.json), split by the recorder's rule as in
    tests/test_gpu_stage3_bf16.py `test_bf16_path_keeps_the_parents_bits`: a digest for every tensor that is not summed with
    atomics and kept its bits over the parent's repeats, the recorded values within the recorder's tolerance for the rest."""
    rec_mod, H = _recorder("record_s3_parent_digests"), _recorder("record_s3_golden")
    with open(os.path.join(golden_dir, "s3_bf16_attn_parent_digests.json")) as f:
        rec = json.load(f)
    got = rec_mod.step_tensors(torch, "s384x2", "mp3")
    want, varies = rec["cases"]["s384x2"], rec["varies"]["s384x2"]
    assert set(got) == set(want) | set(varies) and all(H.is_atomic(k) or k in rec["observed"]["s384x2"] for k in varies)
    assert "grads.blocks.0.attn.qkv.weight" in want
    wrong = [k for k in want if H.digest(got[k]) != want[k]]
    assert not wrong, wrong
    for k, r in varies.items():
        values, spread = H.unpack(torch, r)
        err = float((got[k] - values).abs().max())
        print(f"  {k}: |got - recorded| {err:.3e}, bound {H.tolerance(values, spread):.3e}")
        assert err <= H.tolerance(values, spread), (k, err, H.tolerance(values, spread))
