"""GPU: stage 3 at another position grid than the checkpoint's -- the two resample kernels (dvt_pos_resample_fwd / _bwd)
alone against float64, one step against float64 autograd through oracle/vit.py's resample, slices, the student features
against the fp32 extractor (which resamples on the host), five AdamW steps, the equal-grid path against the bits recorded
from the parent commit (tests/golden/s3_step_parent.json), and `python -m dvt_amd.stage3` end to end."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import vit as OV
from tests import s3_reference as REF

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24  # unit roundoff of fp32

SHAPES = [(5, 7, 7), (16, 7, 7), (5, 7, 9), (4, 7, 7), (37, 16, 16), (37, 73, 73)]
KERNEL_CASES = [(s, 384) for s in SHAPES] + [(s, d) for d in (768, 1024) for s in ((37, 16, 16), (37, 73, 73))]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def dense64(t, g0):
    return torch.eye(g0, dtype=torch.float64) if t is None else t.double()


def taps(t, axis):
    """Largest count of non-zero entries along `axis` of a table (1 for the identity)."""
    return 1 if t is None else int((t != 0).sum(axis).max())


def dev(t):
    return None if t is None else t.to(DEV)


# ---- the kernels alone -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("has_cls", [0, 1])
@pytest.mark.parametrize("shape,dim", KERNEL_CASES)
def test_resample_forward_vs_float64(shape, dim, has_cls):
    """Reference: float64 einsum with the SAME fp32 tables.  The kernel rounds once per tap (one fma each) in the x pass and
    once per tap in the y pass: within (tx + ty) 2^-24 (|Wy| |P| |Wx|^T) to first order; the bound has 2 to spare."""
    from dvt_amd import s3
    g0, gh, gw = shape
    wy, wx = s3.pos_tables(g0, gh, gw)
    g = torch.Generator().manual_seed(dim + g0 + gh)
    pos = torch.randn(has_cls + g0 * g0, dim, generator=g) * torch.logspace(-2, 2, dim)
    out = torch.full((has_cls + gh * gw, dim), float("nan"), device=DEV)
    got = s3.pos_resample(pos.to(DEV), dev(wy), dev(wx), (gh, gw), has_cls, out=out).cpu()
    again = s3.pos_resample(pos.to(DEV), dev(wy), dev(wx), (gh, gw), has_cls).cpu()
    Wy, Wx, P = dense64(wy, g0), dense64(wx, g0), pos[has_cls:].double().reshape(g0, g0, dim)
    want = torch.einsum("ip,pqc,jq->ijc", Wy, P, Wx).reshape(gh * gw, dim)
    bound = (taps(wx, 1) + taps(wy, 1) + 2) * U * torch.einsum("ip,pqc,jq->ijc", Wy.abs(), P.abs(), Wx.abs()).reshape(gh * gw, dim)
    err = (got[has_cls:].double() - want).abs()
    print(f"resample forward {g0} -> {gh} x {gw}, dim {dim}, cls {has_cls}: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(got[:has_cls], pos[:has_cls])       # the cls row is copied
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))  # two launches, equal bits


@pytest.mark.parametrize("has_cls", [0, 1])
@pytest.mark.parametrize("shape,dim", KERNEL_CASES)
def test_resample_transpose_vs_float64(shape, dim, has_cls):
    """dP = prefill + Wy^T dO Wx in float64 with the same tables; the bound is the forward's with the tables' COLUMN tap
    counts.  The prefill proves the pass accumulates; it is drawn inside +-|Wy|^T |dO| |Wx| elementwise, so that the final
    add's own rounding, 2^-24 |dP| <= 2^-24 * 2 |Wy|^T |dO| |Wx|, is the 2 the bound has to spare."""
    from dvt_amd import s3
    g0, gh, gw = shape
    wy, wx = s3.pos_tables(g0, gh, gw)
    g = torch.Generator().manual_seed(dim + g0 + gw + 1)
    dout = torch.randn(has_cls + gh * gw, dim, generator=g) * torch.logspace(-2, 2, dim)
    Wy, Wx, dO = dense64(wy, g0), dense64(wx, g0), dout[has_cls:].double().reshape(gh, gw, dim)
    mag = torch.einsum("ip,ijc,jq->pqc", Wy.abs(), dO.abs(), Wx.abs()).reshape(g0 * g0, dim)
    pre = torch.cat([torch.randn(has_cls, dim, generator=g),
                     (mag * (1.98 * torch.rand(mag.shape, generator=g, dtype=torch.float64) - 0.99)).float()])
    got = s3.pos_resample_bwd(dout.to(DEV), pre.to(DEV), dev(wy), dev(wx), (gh, gw), has_cls).cpu()
    again = s3.pos_resample_bwd(dout.to(DEV), pre.to(DEV), dev(wy), dev(wx), (gh, gw), has_cls).cpu()
    want = pre[has_cls:].double() + torch.einsum("ip,ijc,jq->pqc", Wy, dO, Wx).reshape(g0 * g0, dim)
    bound = (taps(wx, 0) + taps(wy, 0) + 2) * U * mag
    err = (got[has_cls:].double() - want).abs()
    print(f"resample transpose {gh} x {gw} -> {g0}, dim {dim}, cls {has_cls}: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(got[:has_cls], pre[:has_cls] + dout[:has_cls])   # the cls row's gradient is added straight through
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))


# ---- the step --------------------------------------------------------------------------------------------------
def problem(g0, img_h, img_w, stride=14, batch=2, n_reg=0, dim=384, depth=2, seed=0):
    """A ViT whose position table is g0 x g0, an image batch and a target at the run's grid."""
    from dvt_amd.vit import random_state_dict
    gh, gw = (img_h - 14) // stride + 1, (img_w - 14) // stride + 1
    sd = random_state_dict(dim, depth, 14, (0 if n_reg else 1) + g0 * g0, seed=seed, well_conditioned=True, n_reg=n_reg)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(batch, 3, img_h, img_w, generator=gen)
    t = torch.randn(batch, gh, gw, dim, generator=gen)
    return sd, x, t


def engine_for(sd, g0, img_h, img_w, stride=14, n_reg=0, dim=384, depth=2, **kw):
    from dvt_amd import s3
    eng = s3.Stage3Engine(s3.make_config(dim, depth, 14, stride, img_h, img_w, n_reg), DEV, pos_grid=g0, **kw)
    eng.load_timm(sd)
    return eng


STEP_CASES = [(5, 98, 98, 14, 0), (5, 98, 98, 14, 4), (16, 98, 98, 14, 0), (5, 98, 126, 14, 0), (4, 56, 56, 7, 0)]


@pytest.mark.parametrize("g0,img_h,img_w,stride,n_reg", STEP_CASES)
def test_step_gradients_vs_autograd(g0, img_h, img_w, stride, n_reg):
    """tests/s3_reference.step differentiates through oracle/vit.py's resample; bars of tests/test_gpu_stage3.py."""
    sd, x, t = problem(g0, img_h, img_w, stride, n_reg=n_reg)
    want_f, want_l, want_g = REF.step(sd, x, t, stride=stride)
    eng = engine_for(sd, g0, img_h, img_w, stride, n_reg)
    feat = torch.empty(t.shape, device=DEV)
    loss = eng.train_step(x.to(DEV), t.to(DEV), feat).cpu().tolist()
    grads = eng.views(eng.grads)
    assert tuple(grads["pos_embed"].shape) == tuple(sd["pos_embed"].shape) == (1, (0 if n_reg else 1) + g0 * g0, 384)
    errs = {k: rel(grads[k], want_g[k]) for k in grads}
    worst = max(errs, key=errs.get)
    print(f"stage-3 step, table {g0} at {img_h} x {img_w} stride {stride} reg {n_reg}: worst {worst} {errs[worst]:.2e}, "
          f"pos_embed {errs['pos_embed']:.2e}, features {rel(feat, want_f):.2e}, loss {loss[0]:.7f} vs {want_l[0]:.7f}")
    for got, want in zip(loss[:3], want_l):
        assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (loss, want_l)
    assert rel(feat, want_f) < 1e-5
    assert set(errs) == set(want_g) and all(v < 3e-5 for v in errs.values()), errs


def test_slices_equal_whole_batch():
    sd, x, t = problem(5, 98, 98, batch=4, seed=5)
    whole = engine_for(sd, 5, 98, 98)
    lw = whole.train_step(x.to(DEV), t.to(DEV)).cpu()
    sliced = engine_for(sd, 5, 98, 98)
    ls = sliced.train_step(x.to(DEV), t.to(DEV), micro_batch=2).cpu()
    assert rel(ls[:3], lw[:3]) < 1e-5
    gw, gs = whole.views(whole.grads), sliced.views(sliced.grads)
    errs = {k: rel(gs[k], gw[k]) for k in gw}
    print(f"stage-3 slices at table 5 -> 7 x 7: pos_embed {errs['pos_embed']:.2e}, worst {max(errs.values()):.2e}")
    assert all(v < 1e-5 for v in errs.values()), errs


def test_features_equal_fp32_extractor():
    from dvt_amd.vit import HipViT
    sd, x, t = problem(5, 98, 98, seed=3)
    eng = engine_for(sd, 5, 98, 98)
    feat = torch.empty(t.shape, device=DEV)
    eng.train_step(x.to(DEV), t.to(DEV), feat)
    want = HipViT(sd, 14, 14, (98, 98), DEV, dtype="float32").forward_features(x.to(DEV))
    cos = torch.nn.functional.cosine_similarity(feat.reshape(-1, 384), want.reshape(-1, 384), dim=-1)
    err = float(((feat - want).abs().max() / want.abs().max()).cpu())
    print(f"stage-3 features vs dvt_vit_forward_f32 (ViT-S, 2 blocks, table 5 at 98): min cosine {cos.min():.8f}, max rel {err:.2e}")
    assert cos.min() >= 0.999999 and err <= 1e-5


def test_short_run_follows_torch_adamw():
    """The checkpoint-shaped table itself is what AdamW steps."""
    from dvt_amd.stage2 import CosineScheduler
    sd, x, t = problem(5, 98, 98, seed=7)
    steps, wd = 5, 1e-5
    sched = CosineScheduler(2e-4, 1e-6, steps, warmup_iters=int(0.15 * steps) or 1, start_warmup_value=0)
    p = REF.leaves(sd)
    opt = torch.optim.AdamW(list(p.values()), lr=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    eng = engine_for(sd, 5, 98, 98)
    gen = torch.Generator().manual_seed(11)
    for i in range(steps):
        xi = x + 0.1 * torch.randn(x.shape, generator=gen)
        lr = float(sched[i])
        for gr in opt.param_groups:
            gr["lr"] = lr
        opt.zero_grad()
        loss, _, _ = REF.loss_fn(OV.forward_features(p, xi.double(), patch=14, stride=14), t.double())
        loss.backward()
        opt.step()
        eng.train_step(xi.to(DEV), t.to(DEV))
        eng.adamw_step(lr, wd)
    got = eng.views()
    assert tuple(got["pos_embed"].shape) == (1, 26, 384)
    errs = {k: rel(got[k], p[k]) for k in got}
    worst = max(errs, key=errs.get)
    print(f"stage-3 five AdamW steps at table 5 -> 7 x 7: worst {worst} {errs[worst]:.2e}, pos_embed {errs['pos_embed']:.2e}")
    assert all(v < 1e-4 for v in errs.values()), errs


# ---- the equal grid is untouched -------------------------------------------------------------------------------
def _recorder():
    spec = importlib.util.spec_from_file_location("record_s3_golden", os.path.join(ROOT, "tools", "record_s3_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("entry", ["old", "pos"])
@pytest.mark.parametrize("case", ["reg0", "reg4"])
def test_equal_grid_bits_equal_the_parent(golden_dir, case, entry):
    """One step of problem(384, 2, 98, 2) through the entry points without a position grid ("old") and through the `_pos`
    ones called with g0 = the run's 7 ("pos"), against what tools/record_s3_golden.py recorded from the parent commit.
    Features and every gradient whose reduction has a fixed order -- the matrices, the biases, the tokens, pos_embed -- must
    have the parent's bits.  The loss and the LayerNorm / LayerScale parameter gradients are summed with float atomics; the
    parent did not reproduce their bits over its own 16 repeats (largest distance from the first repeat: `spread`), so they
    are held to the recorded values within the recorder's `tolerance` (twice that spread)."""
    rec_mod = _recorder()
    with open(os.path.join(golden_dir, "s3_step_parent.json")) as f:
        rec = json.load(f)
    got = rec_mod.step_tensors(torch, rec_mod.CASES[case], **({} if entry == "old" else {"pos_grid": 7}))
    want, varies = rec["cases"][case], rec["varies"][case]
    assert set(got) == set(want) | set(varies) and "feat" in want and "grads.pos_embed" in want
    wrong = [k for k in want if rec_mod.digest(got[k]) != want[k]]
    assert not wrong, wrong
    for k, r in varies.items():
        values, spread = rec_mod.unpack(torch, r)
        tol = rec_mod.tolerance(values, spread)
        err = float((got[k] - values).abs().max())
        assert err <= tol, (k, err, tol)


# ---- the driver ------------------------------------------------------------------------------------------------
def _image_folder(root):
    from PIL import Image
    rng = np.random.default_rng(0)
    sizes = {"a": [(60, 80), (120, 90)], "b": [(98, 98), (50, 140), (77, 66)]}
    for cls, dims in sizes.items():
        os.makedirs(os.path.join(root, cls), exist_ok=True)
        for i, (h, w) in enumerate(dims):
            Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, cls, f"{i}.png"))


def test_driver_end_to_end(tmp_path, capsys):
    """A ViT checkpoint and a denoiser checkpoint at 5 x 5, a run at 98 x 98 (7 x 7)."""
    from dvt_amd import stage2, stage3
    from dvt_amd.models import Denoiser
    from dvt_amd.models.vit_wrapper import PretrainedViTWrapper
    from dvt_amd.vit import random_state_dict
    root, dim = str(tmp_path), 384
    _image_folder(f"{root}/images")
    torch.save(random_state_dict(dim, 12, 14, 1 + 25, seed=4, well_conditioned=True), f"{root}/vit_s.pth")
    den = Denoiser(5, 5, dim, None, num_blocks=1, device=DEV, seed=0)
    os.makedirs(f"{root}/s2/checkpoints")
    stage2.save_checkpoint(f"{root}/s2", den, 0, 1e-4, 1e-5)
    del den
    args = stage3.get_args(["--model", "vit_small_patch14_dinov2.lvd142m", "--denoiser_ckpt",
                            f"{root}/s2/checkpoints/ckpt_000000.pth", "--data_root", f"{root}/images", "--input_size", "98",
                            "98", "--auto_stride", "--batch_size", "2", "--num_iterations", "3", "--save_freq", "2",
                            "--log_freq", "1", "--num_workers", "2", "--output_root", f"{root}/work",
                            "--vit_checkpoint", f"{root}/vit_s.pth"])
    seen = []

    def factory(a, device):
        eng, teacher = stage3.build_models(a, device)
        assert teacher.noise_map_size == (5, 5) and eng.pos_grid == 5

        def recording_teacher(img, return_dict=True):
            out = teacher(img, return_dict=return_dict)
            seen.append((img.detach().cpu().clone(), out["denoised_feats"].detach().cpu().clone()))
            return out
        return eng, recording_teacher

    out = stage3.train(args, 0, 1, DEV, model_factory=factory)
    assert "position table 5 x 5 resampled to 7 x 7 in every step" in capsys.readouterr().out
    losses = [h["loss"] for h in out["history"]]
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
    assert all(tuple(tgt.shape) == (2, 7, 7, dim) for _, tgt in seen)
    ck_dir = f"{root}/work/denosing-vit/debug/checkpoints"
    ck = torch.load(f"{ck_dir}/latest.pth", weights_only=False)
    assert ck["step"] == 2 and tuple(ck["model"]["model.pos_embed"].shape) == (1, 26, dim)
    assert tuple(ck["optimizer"]["state"][list(ck["model"]).index("model.pos_embed")]["exp_avg"].shape) == (1, 26, dim)
    sd0 = torch.load(f"{root}/vit_s.pth")
    assert not torch.equal(ck["model"]["model.pos_embed"], sd0["pos_embed"])  # the table itself was trained
    # the distilled checkpoint goes back into the wrapper at the run's geometry; its fp32 features are the engine's
    w = PretrainedViTWrapper("vit_small_patch14_dinov2.lvd142m", stride=14, checkpoint_path=f"{ck_dir}/latest.pth",
                             img_size=(98, 98), dtype="float32")
    img, tgt = seen[0]
    feat = torch.empty(tgt.shape, device=DEV)
    out["engine"].train_step(img.to(DEV), tgt.to(DEV), feat)
    ref = w.features_nhwc(img.to(DEV))
    cos = torch.nn.functional.cosine_similarity(feat.reshape(-1, dim), ref.reshape(-1, dim), dim=-1)
    err = float(((feat - ref).abs().max() / ref.abs().max()).cpu())
    print(f"stage-3 driver at table 5 -> 7 x 7: losses {losses}, wrapper vs engine min cosine {cos.min():.8f}, max rel {err:.2e}")
    assert cos.min() >= 0.999999 and err <= 1e-5
