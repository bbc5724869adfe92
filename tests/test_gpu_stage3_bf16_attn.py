"""GPU: the stage-3 step with bf16 GEMMs AND the bf16 flash attention (include/dvt_stage3.h, gemm_mode 3;
`Stage3Engine(dtype="bfloat16", attention="bfloat16")`, `python -m dvt_amd.stage3 --dtype bfloat16 --attention bfloat16`) at the
shapes of tests/test_gpu_stage3_bf16.py: one step against float64 autograd with the whole-step comparator of
tests/s3_attn_reference.py as the yardstick (the rule of that file: at most 2 x the comparator's own distance, per tensor),
proof that the mode is engaged, slices against the whole batch, a short AdamW run, and the driver."""
import functools
import math
import os

import pytest
import torch

from tests import s3_attn_reference as ATT
from tests import s3_bf16_reference as MP
from tests import s3_reference as REF
from tests.test_gpu_stage3_bf16 import DEV, SHAPES, _image_folder, engine_for, problem, rel

pytestmark = pytest.mark.gpu
BF16 = dict(dtype="bfloat16", attention="bfloat16")


@functools.lru_cache(maxsize=None)
def references(shape):
    """(float64 autograd, the mode's comparator) of one step at `shape`, each (features, loss triple, gradients)."""
    dim, depth, img, batch, n_reg = shape
    sd, x, t = problem(dim, depth, img, batch, n_reg)
    return REF.step(sd, x, t), ATT.step(sd, x, t)


@functools.lru_cache(maxsize=None)
def gpu_step(shape, attention):
    dim, depth, img, batch, n_reg = shape
    sd, x, t = problem(dim, depth, img, batch, n_reg)
    eng = engine_for(sd, dim, depth, img, n_reg, dtype="bfloat16", attention=attention)
    feat = torch.empty(t.shape, device=DEV)
    loss = eng.train_step(x.to(DEV), t.to(DEV), feat).cpu().clone()
    return loss, feat.cpu(), {k: v.cpu().clone() for k, v in eng.views(eng.grads).items()}


@pytest.mark.parametrize("shape", SHAPES)
def test_step_gradients_vs_float64(shape):
    """Per parameter tensor, the features and the loss triple: relative-L2 distance from float64 autograd <= 2 x the
    comparator's."""
    (f64_f, f64_l, f64_g), (cmp_f, cmp_l, cmp_g) = references(shape)
    loss, feat, grads = gpu_step(shape, "bfloat16")
    assert set(grads) == set(f64_g)
    ratios = {}
    for k in sorted(grads):
        got, yard = rel(grads[k], f64_g[k]), rel(cmp_g[k], f64_g[k])
        ratios[k] = got / yard
        print(f"  {shape} {k}: step {got:.3e}, comparator {yard:.3e}, ratio {ratios[k]:.3f}")
    worst = max(ratios, key=ratios.get)
    got_l, yard_l = rel(loss[:3], torch.tensor(f64_l)), rel(torch.tensor(cmp_l), torch.tensor(f64_l))
    print(f"stage-3 bf16 + bf16 attention step vs float64 {shape}: worst ratio {ratios[worst]:.3f} ({worst}); features "
          f"{rel(feat, f64_f):.3e} vs comparator {rel(cmp_f, f64_f):.3e}; loss triple {got_l:.3e} vs comparator {yard_l:.3e}")
    assert rel(feat, f64_f) <= 2 * rel(cmp_f, f64_f)
    # the k third of every qkv bias gradient: identically zero in exact arithmetic, and the mode adds nothing to it
    dim = shape[0]
    assert all(not grads[k][dim:2 * dim].any() and grads[k][:dim].any() and grads[k][2 * dim:].any()
               for k in grads if k.endswith("attn.qkv.bias"))
    bad = {k: v for k, v in ratios.items() if not v <= 2.0}
    assert not bad, bad
    assert got_l <= 2 * yard_l, (loss.tolist(), f64_l, cmp_l)


def test_mode_is_engaged():
    """Against a silent fallback to the fp32 attention: every gradient of block 0 differs in bits from the bf16-GEMM step's
    (mode 1) on the same input.  Printed beside it: how far block 0's qkv weight gradient moved, and how far the CPU
    comparators with and without the attention's roundings are apart (the magnitudes are held by the test above)."""
    shape, k = SHAPES[0], "blocks.0.attn.qkv.weight"
    dim, depth, img, batch, n_reg = shape
    sd, x, t = problem(dim, depth, img, batch, n_reg)
    g3, g1 = gpu_step(shape, "bfloat16")[2], gpu_step(shape, "float32")[2]
    yard = rel(references(shape)[1][2][k], MP.step(sd, x, t)[2][k])
    print(f"stage-3 mode 3 vs mode 1, {k}: {rel(g3[k], g1[k]):.3e}; comparator with vs without the attention's roundings "
          f"{yard:.3e}")
    same = [n for n in g3 if n.startswith("blocks.0.") and torch.equal(g3[n].view(torch.int32), g1[n].view(torch.int32))]
    assert not same, same


def test_slices_equal_whole_batch():
    """Batch 4 at once and as 2 + 2 normalised by 4: each slice rounds the same weights and rows and no kernel of the mode
    reduces across images, so the bar is the fp32 bound of tests/test_gpu_stage3_bf16.py `test_slices_equal_whole_batch`,
    1e-5.  Measured on an MI355X: loss 2.6e-7, worst gradient 7.9e-8."""
    sd, x, t = problem(384, 2, 98, 4, seed=5)
    whole = engine_for(sd, 384, 2, 98, **BF16)
    lw = whole.train_step(x.to(DEV), t.to(DEV)).cpu()
    sliced = engine_for(sd, 384, 2, 98, **BF16)
    ls = sliced.train_step(x.to(DEV), t.to(DEV), micro_batch=2).cpu()
    gw, gs = whole.views(whole.grads), sliced.views(sliced.grads)
    errs = {k: rel(gs[k], gw[k]) for k in gw}
    print(f"stage-3 bf16 attention slices vs whole batch: loss {rel(ls[:3], lw[:3]):.2e}, worst gradient {max(errs.values()):.2e}")
    assert rel(ls[:3], lw[:3]) < 1e-5
    assert all(v < 1e-5 for v in errs.values()), errs


def test_short_run_follows_comparator_adamw():
    """Five AdamW steps (schedule and inputs of tests/test_gpu_stage3_bf16.py `test_short_run_follows_comparator_adamw`) of the
    engine against the comparator stepped by torch.optim.AdamW; the bar is set as there: per parameter tensor, the distance
    from the comparator is at most the larger of (a) 2 x the distance at which the fp32 engine follows float64 autograd in the
    same run and (b) the comparator's own distance from float64 autograd, both measured here.
    Measured on an MI355X (worst tensor each): fp32 engine against float64 autograd 3.2e-5, comparator against float64
    autograd 5.0e-4, engine against the comparator 1.9e-4; the largest held / bound is 0.66 (`norm.weight`); the two qkv
    biases are held at 1.7e-5 and 1.9e-5 against bars of 6.5e-5 and 3.6e-5.

    The qkv biases are why the mode adds nothing to the k third of a qkv bias gradient (include/dvt_stage3.h).  That third has
    NO gradient -- a softmax row does not change when all its logits move together, float64 autograd gives 1e-17 there --
    but under the attention's roundings sum_k dS[q, k] is no longer zero, and a step that accumulated the residue handed AdamW
    a k-bias gradient of pure rounding noise (0.5 % of the q-bias gradient's norm), which AdamW, dividing by the gradient's own
    magnitude, turned into a walk of about one learning rate per step.  The noise is not reproducible -- a comparator that
    kept it, on inputs moved by 1e-7 relative, gave a k-bias gradient 1.3 norms away from its own (CPU) -- so engine and
    comparator ended sqrt(2) walks apart: 1.15e-3 and 9.9e-4 against bars of 7.8e-4 and 7.9e-4, measured before the mode
    dropped the residue.  Now the engine writes that third's exact value, zero, the comparator models the same
    (`ATT.qkv_bias`), and `test_step_gradients_vs_float64` holds the engine's k third to exactly zero."""
    from dvt_amd.stage2 import CosineScheduler
    from oracle import vit as OV
    sd, x, t = problem(384, 2, 98, 2, seed=7)
    steps, wd = 5, 1e-5
    sched = CosineScheduler(2e-4, 1e-6, steps, warmup_iters=int(0.15 * steps) or 1, start_warmup_value=0)
    p64, pmp = REF.leaves(sd), REF.leaves(sd)
    opts = [torch.optim.AdamW(list(p.values()), lr=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd) for p in (p64, pmp)]
    e32, e16 = engine_for(sd, 384, 2, 98), engine_for(sd, 384, 2, 98, **BF16)
    gen = torch.Generator().manual_seed(11)
    for i in range(steps):
        xi = x + 0.1 * torch.randn(x.shape, generator=gen)
        lr = float(sched[i])
        for opt in opts:
            for gr in opt.param_groups:
                gr["lr"] = lr
            opt.zero_grad()
        REF.loss_fn(OV.forward_features(p64, xi.double(), patch=14, stride=14), t.double())[0].backward()
        REF.loss_fn(ATT.forward_features(pmp, xi.double(), 14, 14), t.double())[0].backward()
        for opt in opts:
            opt.step()
        for eng in (e32, e16):
            eng.train_step(xi.to(DEV), t.to(DEV))
            eng.adamw_step(lr, wd)
    v32, v16 = e32.views(), e16.views()
    d32 = {k: rel(v32[k], p64[k]) for k in v32}
    dcmp = {k: rel(pmp[k], p64[k]) for k in v32}
    d16 = {k: rel(v16[k], pmp[k]) for k in v32}
    print(f"stage-3 five AdamW steps, bf16 attention: fp32 engine vs float64 worst {max(d32.values()):.2e}; comparator vs float64 "
          f"worst {max(dcmp.values()):.2e}; engine vs comparator worst {max(d16.values()):.2e}; worst held/bound "
          f"{max(d16[k] / max(2 * d32[k], dcmp[k]) for k in d16):.3f} "
          f"({max(d16, key=lambda k: d16[k] / max(2 * d32[k], dcmp[k]))}); qkv biases held, fp32, comparator "
          f"{[(d16[k], d32[k], dcmp[k]) for k in d16 if k.endswith('qkv.bias')]}")
    bad = {k: (d16[k], d32[k], dcmp[k]) for k in d16 if not d16[k] <= max(2 * d32[k], dcmp[k])}
    assert not bad, bad


def _driver_args(root):
    return ["--model", "vit_small_patch14_dinov2.lvd142m", "--denoiser_ckpt", f"{root}/s2/checkpoints/ckpt_000000.pth",
            "--data_root", f"{root}/images", "--input_size", "98", "98", "--auto_stride", "--batch_size", "2",
            "--num_iterations", "2", "--save_freq", "1", "--log_freq", "1", "--num_workers", "2", "--output_root",
            f"{root}/work", "--vit_checkpoint", f"{root}/vit_s.pth"]


def test_driver_bf16_attention(tmp_path, capsys):
    """`stage3.main --dtype bfloat16 --attention bfloat16` for two steps on the tiny image folder of the bf16 driver test: the
    banner names the attention, the losses are finite, the checkpoint has that test's key set in fp32 and it trained.
    `--attention bfloat16` alone exits with the refusal and writes nothing."""
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
    with pytest.raises(SystemExit, match="--attention bfloat16 needs --dtype bfloat16"):
        stage3.main(_driver_args(root) + ["--attention", "bfloat16"])
    assert not os.path.exists(f"{root}/work")
    stage3.main(_driver_args(root) + ["--dtype", "bfloat16", "--attention", "bfloat16"])
    out = capsys.readouterr().out
    assert "student step dtype bfloat16" in out and "student attention bfloat16" in out
    losses = [float(line.split("loss:")[1].split()[0]) for line in out.splitlines() if line.startswith("Train ")]
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses), out
    ck = torch.load(f"{root}/work/denosing-vit/debug/checkpoints/latest.pth", weights_only=False)
    assert set(ck) == {"model", "optimizer", "step"} and set(ck["model"]) == {"model." + k for k in sd}
    assert all(v.dtype == torch.float32 for v in ck["model"].values())
    assert not torch.equal(ck["model"]["model.blocks.0.attn.qkv.weight"], sd["blocks.0.attn.qkv.weight"])
