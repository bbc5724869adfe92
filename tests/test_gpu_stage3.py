"""GPU: the stage-3 distillation step (include/dvt_stage3.h) -- one `dvt_s3_train_step` against float64 autograd through
oracle/vit.py, the student features against the fp32 extractor, slices against the whole batch, a short AdamW run against
torch.optim.AdamW, and the `python -m dvt_amd.stage3` loop end to end.  Tolerances are per-tensor relative L2."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import vit as OV
from tests import s3_reference as REF

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def engine_for(sd, dim, depth, img, stride=14, n_reg=0, **kw):
    from dvt_amd import s3
    cfg = s3.make_config(dim, depth, 14, stride, img, img, n_reg)
    eng = s3.Stage3Engine(cfg, DEV, **kw)
    eng.load_timm(sd)
    return eng


def problem(dim, depth, img, batch, n_reg=0, seed=0):
    from dvt_amd.vit import random_state_dict
    g = (img - 14) // 14 + 1
    sd = random_state_dict(dim, depth, 14, (0 if n_reg else 1) + g * g, seed=seed, well_conditioned=True, n_reg=n_reg)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(batch, 3, img, img, generator=gen)
    t = torch.randn(batch, g, g, dim, generator=gen)
    return sd, x, t


def test_layout_names_and_shapes(built_lib):
    from dvt_amd import s3
    from dvt_amd.vit import random_state_dict
    for n_reg in (0, 4):
        cfg = s3.make_config(384, 3, 14, 14, 98, 98, n_reg)
        total, layout = s3.param_layout(cfg)
        sd = random_state_dict(384, 3, 14, (0 if n_reg else 1) + 49, n_reg=n_reg)
        assert set(layout) == set(sd)
        assert all(tuple(sd[k].shape) == s for k, (_, s) in layout.items())
        offs = sorted(o for o, _ in layout.values())
        assert all(o % 4 == 0 for o in offs) and total % 4 == 0
        ends = sorted((o, o + math.prod(s)) for o, s in layout.values())
        assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:])) and ends[-1][1] <= total


@pytest.mark.parametrize("dim,depth,img,batch,n_reg", [(384, 2, 98, 2, 0), (384, 2, 98, 2, 4), (768, 2, 518, 2, 0)])
def test_step_gradients_vs_autograd(dim, depth, img, batch, n_reg):
    sd, x, t = problem(dim, depth, img, batch, n_reg)
    want_f, want_l, want_g = REF.step(sd, x, t)
    eng = engine_for(sd, dim, depth, img, n_reg=n_reg)
    feat = torch.empty(t.shape, device=DEV)
    loss = eng.train_step(x.to(DEV), t.to(DEV), feat).cpu().tolist()
    for got, want in zip(loss[:3], want_l):
        assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (loss, want_l)
    assert rel(feat, want_f) < 1e-5
    grads = eng.views(eng.grads)
    errs = {k: rel(grads[k], want_g[k]) for k in grads}
    worst = max(errs, key=errs.get)
    print(f"stage-3 step vs float64 autograd ({dim}, {depth}, {img}, reg {n_reg}): worst {worst} {errs[worst]:.2e}, "
          f"loss {loss[0]:.7f} vs {want_l[0]:.7f}")
    assert all(v < 3e-5 for v in errs.values()), errs  # measured: <= 1e-5 at these shapes


def test_features_equal_fp32_extractor():
    from dvt_amd.vit import HipViT
    sd, x, t = problem(768, 12, 518, 1, seed=3)
    eng = engine_for(sd, 768, 12, 518)
    feat = torch.empty(t.shape, device=DEV)
    eng.train_step(x.to(DEV), t.to(DEV), feat)
    want = HipViT(sd, 14, 14, (518, 518), DEV, dtype="float32").forward_features(x.to(DEV))
    cos = torch.nn.functional.cosine_similarity(feat.reshape(-1, 768), want.reshape(-1, 768), dim=-1)
    err = float(((feat - want).abs().max() / want.abs().max()).cpu())
    print(f"stage-3 features vs dvt_vit_forward_f32 (ViT-B/14, 518, 12 blocks): min cosine {cos.min():.8f}, max rel {err:.2e}")
    assert cos.min() >= 0.999999 and err <= 1e-5


def test_slices_equal_whole_batch():
    sd, x, t = problem(384, 2, 98, 4, seed=5)
    whole = engine_for(sd, 384, 2, 98)
    lw = whole.train_step(x.to(DEV), t.to(DEV)).cpu()
    sliced = engine_for(sd, 384, 2, 98)
    ls = sliced.train_step(x.to(DEV), t.to(DEV), micro_batch=2).cpu()
    assert rel(ls[:3], lw[:3]) < 1e-5
    gw, gs = whole.views(whole.grads), sliced.views(sliced.grads)
    errs = {k: rel(gs[k], gw[k]) for k in gw}
    assert all(v < 1e-5 for v in errs.values()), errs
    # a budget below one image is refused with the bytes it needs
    from dvt_amd import _lib
    tiny = engine_for(sd, 384, 2, 98, max_work_bytes=1 << 20)
    with pytest.raises(_lib.DvtError, match="bytes"):
        tiny.train_step(x.to(DEV), t.to(DEV))


def test_short_run_follows_torch_adamw():
    from dvt_amd.stage2 import CosineScheduler
    sd, x, t = problem(384, 2, 98, 2, seed=7)
    steps, wd = 5, 1e-5
    sched = CosineScheduler(2e-4, 1e-6, steps, warmup_iters=int(0.15 * steps) or 1, start_warmup_value=0)
    p = REF.leaves(sd)
    opt = torch.optim.AdamW(list(p.values()), lr=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    eng = engine_for(sd, 384, 2, 98)
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
    errs = {k: rel(got[k], p[k]) for k in got}
    worst = max(errs, key=errs.get)
    print(f"stage-3 five AdamW steps vs torch.optim.AdamW: worst {worst} {errs[worst]:.2e}")
    assert all(v < 1e-4 for v in errs.values()), errs


def _image_folder(root):
    from PIL import Image
    rng = np.random.default_rng(0)
    sizes = {"a": [(60, 80), (120, 90)], "b": [(98, 98), (50, 140), (77, 66)]}
    for cls, dims in sizes.items():
        os.makedirs(os.path.join(root, cls), exist_ok=True)
        for i, (h, w) in enumerate(dims):
            Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, cls, f"{i}.png"))


def test_driver_end_to_end(tmp_path):
    from dvt_amd import stage2, stage3
    from dvt_amd.models import Denoiser
    from dvt_amd.models.vit_wrapper import PretrainedViTWrapper
    from dvt_amd.vit import random_state_dict
    root = str(tmp_path)
    _image_folder(f"{root}/images")
    torch.save(random_state_dict(384, 12, 14, 1 + 49, seed=4, well_conditioned=True), f"{root}/vit_s.pth")
    den = Denoiser(7, 7, 384, None, num_blocks=1, device=DEV, seed=0)
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

        def recording_teacher(img, return_dict=True):
            out = teacher(img, return_dict=return_dict)
            seen.append((img.detach().cpu().clone(), out["denoised_feats"].detach().cpu().clone()))
            return out
        return eng, recording_teacher

    out = stage3.train(args, 0, 1, DEV, model_factory=factory)
    losses = [h["loss"] for h in out["history"]]
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
    # the reference loop on the same batches: float64 autograd + torch.optim.AdamW, sqrt-scaled lr, cosine schedule
    sd = torch.load(f"{root}/vit_s.pth")
    p = REF.leaves(sd)
    opt = torch.optim.AdamW(list(p.values()), betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)
    sched = stage3.scheduler(args, stage3.learning_rate(args, 1), 3)
    want = []
    for step, (img, tgt) in enumerate(seen[:3]):
        for g in opt.param_groups:
            g["lr"] = float(sched[step])
        opt.zero_grad()
        loss, _, _ = REF.loss_fn(OV.forward_features(p, img.double(), patch=14, stride=14), tgt.double())
        loss.backward()
        opt.step()
        want.append(loss.item())
    print(f"stage-3 driver losses {losses} vs reference loop {want}")
    assert np.allclose(losses, want, rtol=1e-5, atol=1e-6), (losses, want)
    ck_dir = f"{root}/work/denosing-vit/debug/checkpoints"
    assert sorted(os.listdir(ck_dir)) == ["ckpt_000000.pth", "ckpt_000002.pth", "latest.pth"]
    ck = torch.load(f"{ck_dir}/latest.pth", weights_only=False)
    assert ck["step"] == 2 and set(ck["model"]) == {"model." + k for k in sd}
    assert "model.blocks.0.ls1.gamma" in ck["model"]
    got = {k[len("model."):]: v for k, v in ck["model"].items()}
    assert max(rel(got[k], p[k]) for k in got) < 1e-4
    # the distilled checkpoint goes straight back into the wrapper; its fp32 features are the engine's student features
    w = PretrainedViTWrapper("vit_small_patch14_dinov2.lvd142m", stride=14, checkpoint_path=f"{ck_dir}/latest.pth",
                             img_size=(98, 98), dtype="float32")
    img, tgt = seen[0]
    feat = torch.empty(tgt.shape, device=DEV)
    out["engine"].train_step(img.to(DEV), tgt.to(DEV), feat)
    ref = w.features_nhwc(img.to(DEV))
    cos = torch.nn.functional.cosine_similarity(feat.reshape(-1, 384), ref.reshape(-1, 384), dim=-1)
    assert cos.min() >= 0.999999 and rel(feat, ref) < 1e-5
