"""GPU: the stage-3 step's opt-in bf16 mode (include/dvt_stage3.h, gemm_mode 1; `Stage3Engine(dtype="bfloat16")`,
`python -m dvt_amd.stage3 --dtype bfloat16`): the casts bit for bit, one step against float64 autograd with the CPU
comparator of tests/s3_bf16_reference.py as the yardstick, proof that the mode is engaged, the default path's bits against the
parent commit's, slices against the whole batch, a short AdamW run, and the driver.

The yardstick is never the code under test: the comparator evaluates the mode's arithmetic (bf16 operands in the forward and
data-gradient products of the four linear layers, everything else exact) in float64, so its distance from plain float64
autograd is what the ROUNDING costs; the kernels may add their fp32 accumulation to that, hence the factor 2 (the rule of
tests/test_gpu_fit_grads.py)."""
import functools
import hashlib
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import s3_bf16_reference as MP
from tests import s3_reference as REF

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(384, 2, 98, 2, 0), (384, 2, 98, 2, 4), (768, 1, 98, 2, 0)]  # (dim, depth, img, batch, n_reg): 7 x 7 tokens, s_pad 128


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def problem(dim, depth, img, batch, n_reg=0, seed=0):
    from dvt_amd.vit import random_state_dict
    g = (img - 14) // 14 + 1
    sd = random_state_dict(dim, depth, 14, (0 if n_reg else 1) + g * g, seed=seed, well_conditioned=True, n_reg=n_reg)
    gen = torch.Generator().manual_seed(seed + 1)
    return sd, torch.randn(batch, 3, img, img, generator=gen), torch.randn(batch, g, g, dim, generator=gen)


def engine_for(sd, dim, depth, img, n_reg=0, **kw):
    from dvt_amd import s3
    eng = s3.Stage3Engine(s3.make_config(dim, depth, 14, 14, img, img, n_reg), DEV, **kw)
    eng.load_timm(sd)
    return eng


@functools.lru_cache(maxsize=None)
def references(shape):
    """(float64 autograd, comparator) of one step at `shape`, each (features, loss triple, gradients): computed once."""
    dim, depth, img, batch, n_reg = shape
    sd, x, t = problem(dim, depth, img, batch, n_reg)
    return REF.step(sd, x, t), MP.step(sd, x, t)


@functools.lru_cache(maxsize=None)
def gpu_step(shape, dtype):
    """(loss[4], features, {name: gradient}) (CPU) of one step of a fresh engine."""
    dim, depth, img, batch, n_reg = shape
    sd, x, t = problem(dim, depth, img, batch, n_reg)
    eng = engine_for(sd, dim, depth, img, n_reg, dtype=dtype)
    feat = torch.empty(t.shape, device=DEV)
    loss = eng.train_step(x.to(DEV), t.to(DEV), feat).cpu().clone()
    return loss, feat.cpu(), {k: v.cpu().clone() for k, v in eng.views(eng.grads).items()}


# ---- 1. the casts, bit for bit ------------------------------------------------------------------------------------
def cast_values(rows, n, seed):
    """fp32 [rows, n]: random bit patterns over the whole finite range (denormals and huge values included) with the cases a
    rounding can get wrong planted at the front: exact ties above even and odd mantissas, one ulp to either side of a tie,
    +-0, the smallest and largest denormals, the largest bf16 and the finite values around it (those above its tie round to
    infinity, as torch's do), both signs.  No NaN, no infinity in the input."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows * n,), generator=g, dtype=torch.int64).to(torch.int32)
    expo = (bits >> 23) & 0xFF
    bits = torch.where(expo == 0xFF, bits & ~(1 << 23), bits)  # exponent 255 -> 254: finite
    special = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x00000000, 0x00000001, 0x007FFFFF,
               0x00008000, 0x00018000, 0x00007FFF, 0x00800000, 0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0x7F7E8000,
               0x7F000000, 0x4B800000, 0x3F7FFFFF, 0x3F7F8000, 0x0000FFFF, 0x007F8000]
    special = special + [s | 0x80000000 for s in special]
    sp = torch.tensor([s - (1 << 32) if s >= (1 << 31) else s for s in special], dtype=torch.int32)
    bits[:sp.numel()] = sp
    bits[-sp.numel():] = sp  # (and in the last row / the last tile)
    return bits.view(torch.float32).reshape(rows, n)


def as_bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


@pytest.mark.parametrize("rows,n", [(256, 384), (384, 1536)])
def test_row_cast_bits(rows, n):
    from dvt_amd import s3
    x = cast_values(rows, n, rows + n)
    assert torch.isfinite(x).all() and (x == 0).sum() >= 4 and ((x != 0) & (x.abs() < 1.18e-38)).sum() >= 8
    got = s3.cast_bf16(x.to(DEV))
    want = x.to(torch.bfloat16)
    assert torch.isinf(want.float()).any()  # the values above the largest bf16's tie
    assert got.shape == want.shape and torch.equal(as_bits(got), as_bits(want))


@pytest.mark.parametrize("n,k", [(1152, 384), (384, 1536), (64, 64)])
def test_transposed_cast_bits(n, k):
    from dvt_amd import s3
    w = cast_values(n, k, 7 * n + k)
    got = s3.cast_bf16_t(w.to(DEV))
    want = w.to(torch.bfloat16).t().contiguous()
    assert tuple(got.shape) == (k, n) and torch.equal(as_bits(got), as_bits(want))


# ---- 2. one step against float64 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_step_gradients_vs_float64(shape):
    """Per parameter tensor: relative-L2 distance of the bf16 step's gradient from float64 autograd <= 2 x the comparator's
    distance from float64 autograd on the same inputs -- the weight gradients included (their own product is fp32, their
    inputs carry the rounding from upstream) -- and the loss triple [loss, l2, cos] the same way, as one tensor of three.
    (Not element by element: the step and the comparator do not make the SAME rounding errors.  An operand that the fp32
    kernels computed a few ulp away from float64 rounds to the other bf16 neighbour now and then, that moves the next layer's
    operands by far more than fp32 does, and further roundings flip: at the first shape the step's features are 2.4e-3 from
    the comparator's while both are 9.6e-3 from float64.  A tensor's norm is the same for both draws of the noise -- the
    ratios printed below are 0.97 .. 1.04 -- a single scalar's error is whatever its draw was: there the comparator's cosine
    term lands within 1.3e-7 of float64, the step's within 4.6e-6, the l2 terms within 5.1e-5 and 5.9e-5.)"""
    (f64_f, f64_l, f64_g), (cmp_f, cmp_l, cmp_g) = references(shape)
    loss, feat, grads = gpu_step(shape, "bfloat16")
    assert set(grads) == set(f64_g)
    ratios = {}
    for k in sorted(grads):
        got, yard = rel(grads[k], f64_g[k]), rel(cmp_g[k], f64_g[k])
        ratios[k] = got / yard
        print(f"  {shape} {k}: bf16 step {got:.3e}, comparator {yard:.3e}, ratio {ratios[k]:.3f}")
    worst = max(ratios, key=ratios.get)
    yards = [rel(cmp_g[k], f64_g[k]) for k in grads]
    print(f"stage-3 bf16 step vs float64 {shape}: worst ratio {ratios[worst]:.3f} ({worst}); comparator's own distance from "
          f"float64 {min(yards):.2e} .. {max(yards):.2e}; features {rel(feat, f64_f):.3e} vs comparator {rel(cmp_f, f64_f):.3e}"
          f" (step vs comparator {rel(feat, cmp_f):.3e})")
    for name, got, want, yard in zip(("loss", "l2", "cos"), loss.tolist(), f64_l, cmp_l):
        print(f"  {shape} {name}: bf16 step {got:.8f}, float64 {want:.8f}, comparator {yard:.8f}, "
              f"|step - f64| {abs(got - want):.3e}, |comparator - f64| {abs(yard - want):.3e}")
    assert rel(feat, f64_f) <= 2 * rel(cmp_f, f64_f)
    bad = {k: v for k, v in ratios.items() if not v <= 2.0}
    assert not bad, bad
    got_l, yard_l = rel(loss[:3], torch.tensor(f64_l)), rel(torch.tensor(cmp_l), torch.tensor(f64_l))
    print(f"  {shape} loss triple: bf16 step {got_l:.3e}, comparator {yard_l:.3e}, ratio {got_l / yard_l:.3f}")
    assert got_l <= 2 * yard_l, (loss.tolist(), f64_l, cmp_l)


# ---- 3. the mode is engaged ----------------------------------------------------------------------------------------
def test_mode_is_engaged():
    """Against a silent fallback to fp32 and against a grossly wrong product: block 0's qkv weight gradient of the bf16 step
    differs from the fp32 step's in at least one bit, and by as much as the rounding explains -- its relative-L2 distance
    from the fp32 step's lies within a factor 4, either way, of the comparator's distance from float64."""
    shape, k = SHAPES[0], "blocks.0.attn.qkv.weight"
    (_, _, f64_g), (_, _, cmp_g) = references(shape)
    g16, g32 = gpu_step(shape, "bfloat16")[2][k], gpu_step(shape, "float32")[2][k]
    assert not torch.equal(g16.view(torch.int32), g32.view(torch.int32))
    d, yard = rel(g16, g32), rel(cmp_g[k], f64_g[k])
    print(f"stage-3 bf16 vs fp32 step, {k}: {d:.3e}; comparator vs float64 {yard:.3e}; ratio {d / yard:.3f}")
    assert yard / 4 <= d <= 4 * yard


# ---- 4. the default path keeps the parent's bits -------------------------------------------------------------------
def _recorder(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("route", ["step", "mp0"])
@pytest.mark.parametrize("case", ["s384x2", "b768x1"])
def test_default_path_keeps_the_parents_bits(golden_dir, case, route):
    """One exact-fp32 step at the first and third shape above through `dvt_s3_train_step` ("step") and through the new entry
    point with gemm_mode 0 ("mp0"), against what tools/record_s3_parent_digests.py recorded from the parent commit
    (tests/golden/s3_parent_digests.json).  Every gradient whose reduction has a fixed order has the parent's bits (sha256);
    the loss and the LayerNorm / LayerScale gradients are summed with float atomics, which the parent itself does not
    reproduce bit for bit, and are held to the recorded values within the recorder's tolerance (twice the parent's own
    run-to-run spread) -- the split of tests/test_gpu_stage3_grid.py."""
    rec_mod, H = _recorder("record_s3_parent_digests"), _recorder("record_s3_golden")
    with open(os.path.join(golden_dir, "s3_parent_digests.json")) as f:
        rec = json.load(f)
    got = rec_mod.step_tensors(torch, case, route)
    want, varies = rec["cases"][case], rec["varies"][case]
    assert set(got) == set(want) | set(varies) and "grads.blocks.0.attn.qkv.weight" in want and "grads.pos_embed" in want
    wrong = [k for k in want if H.digest(got[k]) != want[k]]
    assert not wrong, wrong
    for k, r in varies.items():
        values, spread = H.unpack(torch, r)
        err = float((got[k] - values).abs().max())
        assert err <= H.tolerance(values, spread), (k, err, H.tolerance(values, spread))


def test_bf16_path_keeps_the_parents_bits(golden_dir):
    """The bf16 mode's routing moved into the block the two trainers share: one gemm_mode 1 step at the first shape against
    what `tools/record_s3_parent_digests.py --bf16` recorded from the commit before that move
    (tests/golden/s3_bf16_parent_digests.json), split by the recorder's rule as above: a digest for every tensor that is
    not summed with atomics and kept its bits over the parent's repeats, the recorded values within twice the parent's own
    spread (4-ulp floor) for the rest."""
    rec_mod, H = _recorder("record_s3_parent_digests"), _recorder("record_s3_golden")
    with open(os.path.join(golden_dir, "s3_bf16_parent_digests.json")) as f:
        rec = json.load(f)
    got = rec_mod.step_tensors(torch, "s384x2", "mp1")
    want, varies = rec["cases"]["s384x2"], rec["varies"]["s384x2"]
    assert set(got) == set(want) | set(varies) and all(H.is_atomic(k) or k in rec["observed"]["s384x2"] for k in varies)
    wrong = [k for k in want if H.digest(got[k]) != want[k]]
    assert not wrong, wrong
    for k, r in varies.items():
        values, spread = H.unpack(torch, r)
        err = float((got[k] - values).abs().max())
        print(f"  {k}: |got - recorded| {err:.3e}, bound {H.tolerance(values, spread):.3e}")
        assert err <= H.tolerance(values, spread), (k, err, H.tolerance(values, spread))


def test_extractor_keeps_the_parents_bits(golden_dir):
    """The bf16 GEMM unit is shared with the extractor: a 2-block ViT-B/14 bf16 forward still gives the bits of
    tests/golden/vitb_2block_parent.json (the route of tests/test_gpu_vitg.py), also AFTER a bf16 stage-3 step has run its
    GEMMs through the same unit in this process."""
    from dvt_amd.vit import HipViT, random_state_dict
    gpu_step(SHAPES[0], "bfloat16")
    with open(os.path.join(golden_dir, "vitb_2block_parent.json")) as f:
        want = json.load(f)["sha256"]
    sd = random_state_dict(768, 2, 14, 1 + 37 * 37, seed=9, well_conditioned=True, n_reg=0)
    x = torch.randn(2, 3, 518, 518, generator=torch.Generator().manual_seed(12)).to(DEV)
    feat, cls = HipViT(sd, 14, 14, (518, 518), DEV, dtype="bfloat16").forward_features(x, return_cls=True)
    h = hashlib.sha256(feat.cpu().numpy().tobytes() + cls.cpu().numpy().tobytes()).hexdigest()
    assert h == want["bfloat16_reg0"]


# ---- 5. slices add up ----------------------------------------------------------------------------------------------
def test_slices_equal_whole_batch():
    """bf16 mode, batch 4 as one call and as two slices of 2 normalised by 4: each slice rounds the same weights and the same
    rows, so the two agree to the fp32 bound of tests/test_gpu_stage3.py `test_slices_equal_whole_batch` (1e-5)."""
    sd, x, t = problem(384, 2, 98, 4, seed=5)
    whole = engine_for(sd, 384, 2, 98, dtype="bfloat16")
    lw = whole.train_step(x.to(DEV), t.to(DEV)).cpu()
    sliced = engine_for(sd, 384, 2, 98, dtype="bfloat16")
    ls = sliced.train_step(x.to(DEV), t.to(DEV), micro_batch=2).cpu()
    gw, gs = whole.views(whole.grads), sliced.views(sliced.grads)
    errs = {k: rel(gs[k], gw[k]) for k in gw}
    print(f"stage-3 bf16 slices vs whole batch: loss {rel(ls[:3], lw[:3]):.2e}, worst gradient {max(errs.values()):.2e}")
    assert rel(ls[:3], lw[:3]) < 1e-5
    assert all(v < 1e-5 for v in errs.values()), errs


# ---- 6. a short run ------------------------------------------------------------------------------------------------
def test_short_run_follows_comparator_adamw():
    """Five AdamW steps (the schedule and inputs of tests/test_gpu_stage3.py `test_short_run_follows_torch_adamw`) of the
    bf16 engine against the comparator stepped by torch.optim.AdamW.  Per parameter tensor, the relative-L2 distance is at
    most the larger of (a) 2 x the distance at which the fp32 engine follows float64 autograd in that same run and (b) the
    comparator's own distance from float64 autograd -- both measured here, on the same inputs.
    Measured on an MI355X (worst tensor each): fp32 engine against float64 autograd 3.3e-5 (so (a) is 6.6e-5 at most),
    comparator against float64 autograd 4.2e-4, bf16 engine against the comparator 1.0e-4; the largest held / bound over the
    tensors is 0.61."""
    from dvt_amd.stage2 import CosineScheduler
    sd, x, t = problem(384, 2, 98, 2, seed=7)
    steps, wd = 5, 1e-5
    sched = CosineScheduler(2e-4, 1e-6, steps, warmup_iters=int(0.15 * steps) or 1, start_warmup_value=0)
    p64, pmp = REF.leaves(sd), REF.leaves(sd)
    opts = [torch.optim.AdamW(list(p.values()), lr=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd) for p in (p64, pmp)]
    e32, e16 = engine_for(sd, 384, 2, 98), engine_for(sd, 384, 2, 98, dtype="bfloat16")
    gen = torch.Generator().manual_seed(11)
    from oracle import vit as OV
    for i in range(steps):
        xi = x + 0.1 * torch.randn(x.shape, generator=gen)
        lr = float(sched[i])
        for opt in opts:
            for gr in opt.param_groups:
                gr["lr"] = lr
            opt.zero_grad()
        REF.loss_fn(OV.forward_features(p64, xi.double(), patch=14, stride=14), t.double())[0].backward()
        REF.loss_fn(MP.forward_features(pmp, xi.double(), 14, 14), t.double())[0].backward()
        for opt in opts:
            opt.step()
        for eng in (e32, e16):
            eng.train_step(xi.to(DEV), t.to(DEV))
            eng.adamw_step(lr, wd)
    v32, v16 = e32.views(), e16.views()
    d32 = {k: rel(v32[k], p64[k]) for k in v32}    # (a)/2: the fp32 engine against float64 autograd
    dcmp = {k: rel(pmp[k], p64[k]) for k in v32}   # (b): the comparator against float64 autograd
    d16 = {k: rel(v16[k], pmp[k]) for k in v32}    # held: the bf16 engine against the comparator
    print(f"stage-3 five AdamW steps: fp32 engine vs float64 worst {max(d32.values()):.2e}; comparator vs float64 worst "
          f"{max(dcmp.values()):.2e}; bf16 engine vs comparator worst {max(d16.values()):.2e}; worst held/bound "
          f"{max(d16[k] / max(2 * d32[k], dcmp[k]) for k in d16):.3f}")
    bad = {k: (d16[k], d32[k], dcmp[k]) for k in d16 if not d16[k] <= max(2 * d32[k], dcmp[k])}
    assert not bad, bad


# ---- 7. the driver -------------------------------------------------------------------------------------------------
def _image_folder(root):
    from PIL import Image
    rng = np.random.default_rng(0)
    sizes = {"a": [(60, 80), (120, 90)], "b": [(98, 98), (50, 140), (77, 66)]}
    for cls, dims in sizes.items():
        os.makedirs(os.path.join(root, cls), exist_ok=True)
        for i, (h, w) in enumerate(dims):
            Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, cls, f"{i}.png"))


def test_driver_bf16(tmp_path, capsys):
    """`stage3.main --dtype bfloat16` on the tiny image folder of tests/test_gpu_stage3.py's driver test: finite logged
    losses, an fp32 checkpoint in the reference's format that the wrapper loads."""
    from dvt_amd import stage2, stage3
    from dvt_amd.models import Denoiser
    from dvt_amd.models.vit_wrapper import PretrainedViTWrapper
    from dvt_amd.vit import random_state_dict
    root = str(tmp_path)
    _image_folder(f"{root}/images")
    sd = random_state_dict(384, 12, 14, 1 + 49, seed=4, well_conditioned=True)
    torch.save(sd, f"{root}/vit_s.pth")
    den = Denoiser(7, 7, 384, None, num_blocks=1, device=DEV, seed=0)
    os.makedirs(f"{root}/s2/checkpoints")
    stage2.save_checkpoint(f"{root}/s2", den, 0, 1e-4, 1e-5)
    del den
    stage3.main(["--model", "vit_small_patch14_dinov2.lvd142m", "--denoiser_ckpt", f"{root}/s2/checkpoints/ckpt_000000.pth",
                 "--data_root", f"{root}/images", "--input_size", "98", "98", "--auto_stride", "--batch_size", "2",
                 "--num_iterations", "3", "--save_freq", "2", "--log_freq", "1", "--num_workers", "2", "--output_root",
                 f"{root}/work", "--vit_checkpoint", f"{root}/vit_s.pth", "--dtype", "bfloat16"])
    out = capsys.readouterr().out
    assert "student step dtype bfloat16" in out
    losses = [float(line.split("loss:")[1].split()[0]) for line in out.splitlines() if line.startswith("Train ")]
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses), out
    ck_dir = f"{root}/work/denosing-vit/debug/checkpoints"
    assert sorted(os.listdir(ck_dir)) == ["ckpt_000000.pth", "ckpt_000002.pth", "latest.pth"]
    ck = torch.load(f"{ck_dir}/latest.pth", weights_only=False)
    assert set(ck) == {"model", "optimizer", "step"} and ck["step"] == 2 and set(ck["model"]) == {"model." + k for k in sd}
    assert all(v.dtype == torch.float32 for v in ck["model"].values())
    assert not torch.equal(ck["model"]["model.blocks.0.attn.qkv.weight"], sd["blocks.0.attn.qkv.weight"])  # it trained
    w = PretrainedViTWrapper("vit_small_patch14_dinov2.lvd142m", stride=14, checkpoint_path=f"{ck_dir}/latest.pth",
                             img_size=(98, 98), dtype="float32")
    assert all(torch.equal(w._state_dict[k], ck["model"]["model." + k]) for k in sd)
    feats = w.features_nhwc(torch.randn(1, 3, 98, 98, generator=torch.Generator().manual_seed(1)).to(DEV))
    assert tuple(feats.shape) == (1, 7, 7, 384) and torch.isfinite(feats).all()
