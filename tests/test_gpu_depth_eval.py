"""GPU: the cls token of the HIP ViT and the linear-probe depth head and evaluation (csrc/dvt_depth.hip via dvt_amd.depth)
against the float64 restatement in tests/depth_reference.py: the training step (both losses, dW, db), the batch without a
valid pixel, determinism, clipping, AdamW under the cosine / one-cycle schedules, and flip-averaged inference with the
nine metrics."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vit as ovit
from tests import depth_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return ((got - want).norm() / want.norm()).item()


# ---------------------------------------------------------------------------------------------------- cls token
# tolerances: those of the whole-forward patch-token tests of tests/test_gpu_vit.py for the same precision
@pytest.mark.parametrize("mode,cos_min,err_max", [(("bfloat16", "highest"), 0.999, 2e-2), (("float32", "highest"), 0.999999, 2e-5),
                                                  (("float32", "high"), 0.999999, 1e-4)])
@pytest.mark.parametrize("dim,depth,img,n_reg", [(128, 2, 56, 0), (256, 2, 98, 4)])
def test_cls_token_vs_oracle(built_lib, mode, cos_min, err_max, dim, depth, img, n_reg):
    from dvt_amd.vit import HipViT, random_state_dict
    g0 = img // 14
    sd = random_state_dict(dim, depth, 14, (0 if n_reg else 1) + g0 * g0, seed=dim + 3, well_conditioned=True, n_reg=n_reg)
    x = torch.randn(3, 3, img, img, generator=torch.Generator().manual_seed(5))
    stream = []
    ovit.forward_features(sd, x, 14, 14, stream_out=stream)
    want = F.layer_norm(stream[0][:, 0], (dim,), sd["norm.weight"], sd["norm.bias"], 1e-6)
    vit = HipViT(sd, 14, 14, (img, img), DEV, dtype=mode[0], matmul=mode[1])
    plain = vit.forward_features(x.to(DEV)).clone()
    feats, cls = vit.forward_features(x.to(DEV), return_cls=True)
    assert torch.equal(plain, feats), "patch tokens changed with return_cls"
    assert cls.shape == (3, dim) and cls.dtype == torch.float32
    cls = cls.cpu()
    cos = F.cosine_similarity(cls, want, dim=-1)
    err = float((cls - want).norm() / want.norm())
    print(f"cls {mode} dim={dim} reg={n_reg}: cos min {cos.min():.8f} rel-L2 {err:.2e}")
    assert cos.min() > cos_min and err < err_max
    # launches of one view each: same bits
    f1, c1 = vit.forward_features(x.to(DEV), return_cls=True, max_batch=1)
    assert torch.equal(c1.cpu(), cls) and torch.equal(f1, feats)


def test_backbone_returns_cls(built_lib):
    from dvt_amd.seg import ViTBackbone
    from dvt_amd.vit import random_state_dict
    sd = random_state_dict(128, 2, 14, 1 + 16, seed=2, well_conditioned=True)
    img = torch.randn(2, 3, 50, 60, device=DEV)
    f0 = ViTBackbone(sd, 14, DEV)(img)
    f1, cls = ViTBackbone(sd, 14, DEV, return_cls=True)(img)
    assert torch.equal(f0, f1) and cls.shape == (2, 128) and f1.shape == (2, 4, 5, 128)


# ---------------------------------------------------------------------------------------------------- head step
def make_head(C, seed):
    from dvt_amd.depth import DepthHeadEngine
    eng = DepthHeadEngine(C, DEV, seed=seed)
    eng.views()["conv_depth.weight"].mul_(3.0)  # logits of order one on both sides of the relu
    return eng


def make_batch(B, h, w, C, H, W, seed, invalid_image=None, all_invalid=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, h, w, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + 0.3 * torch.randn(C, generator=g)
    cls = torch.randn(B, C, generator=g)
    gt = 0.5 + 8.0 * torch.rand(B, H, W, generator=g)
    gt[torch.rand(B, H, W, generator=g) < 0.1] = 0.0  # ~10 % invalid
    gt[:, :3] = 0.0  # an invalid border, as the rotation and the sensor leave it
    gt[:, :, W - 4:] = 0.0
    if invalid_image is not None:
        gt[invalid_image] = 0.0
    if all_invalid:
        gt[:] = 0.0
    return x.to(DEV).contiguous(), cls.to(DEV).contiguous(), gt.to(DEV).contiguous()


def reference_step(eng, x, cls, gt, warm_up):
    v = eng.views()
    return ref.step_reference(v["conv_depth.weight"].cpu(), v["conv_depth.bias"].cpu(), x.cpu(), cls.cpu(), gt.cpu(), warm_up)


def check_step(eng, x, cls, gt, it, tag):
    want_ld, want_lg, want_dW, want_db = reference_step(eng, x, cls, gt, it < 100)
    out = eng.train_step(x, cls, gt, it).cpu()
    g = eng.views(eng.grads)
    e = {"loss_depth": abs(out[0].item() - want_ld) / abs(want_ld), "dW": rel(g["conv_depth.weight"], want_dW),
         "db": rel(g["conv_depth.bias"], want_db)}
    if want_lg != 0.0:
        e["loss_grad"] = abs(out[1].item() - want_lg) / abs(want_lg)
    print(f"{tag}: loss_depth {out[0].item():.6f} loss_grad {out[1].item():.6f} " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    if want_lg == 0.0:
        assert out[1].item() == 0.0
    assert max(e.values()) < 1e-5, e
    return out, want_lg


@pytest.mark.parametrize("it", [0, 100])
@pytest.mark.parametrize("B", [1, 2, 3, 5])
@pytest.mark.parametrize("C", [384, 768])
def test_head_step_matches_autograd(built_lib, C, B, it):
    h, w, H, W = 9, 11, 45, 61  # label size not a multiple of the grid
    eng = make_head(C, seed=C + B)
    x, cls, gt = make_batch(B, h, w, C, H, W, seed=B + it)
    out, want_lg = check_step(eng, x, cls, gt, it, f"C {C} B {B} it {it}")
    if B <= 2:
        assert out[1].item() == 0.0 and want_lg == 0.0
    else:
        assert want_lg > 0.0


@pytest.mark.parametrize("B,bad", [(2, 1), (3, 1), (5, 2)])
def test_one_image_entirely_invalid(built_lib, B, bad):
    eng = make_head(384, seed=B)
    x, cls, gt = make_batch(B, 9, 11, 384, 45, 61, seed=40 + B, invalid_image=bad)
    check_step(eng, x, cls, gt, 100, f"B {B}, image {bad} invalid")


def test_head_step_at_the_training_geometry(built_lib):
    """samples_per_gpu 2, a 416 x 544 crop: 30 x 39 tokens after the centre padding to 420 x 546."""
    eng = make_head(768, seed=7)
    x, cls, gt = make_batch(2, 30, 39, 768, 416, 544, seed=11)
    check_step(eng, x, cls, gt, 100, "training geometry")


def test_all_invalid_batch(built_lib):
    eng = make_head(384, seed=1)
    x, cls, gt = make_batch(2, 9, 11, 384, 45, 61, seed=3, all_invalid=True)
    eng.grads.fill_(7.0)
    for it in (0, 100):
        out = eng.train_step(x, cls, gt, it).cpu()
        assert torch.isnan(out[0]) and out[1].item() == 0.0
        assert bool((eng.grads == 0).all())


def test_step_is_deterministic_and_ignores_workspace_contents(built_lib):
    eng = make_head(768, seed=5)
    x, cls, gt = make_batch(3, 9, 11, 768, 45, 61, seed=9)
    out1 = eng.train_step(x, cls, gt, 100).clone()
    g1 = eng.grads.clone()
    out2 = eng.train_step(x, cls, gt, 100).clone()
    assert torch.equal(out1, out2) and torch.equal(g1, eng.grads)
    eng._work.view(torch.float32)[:] = float("nan")
    eng.grads.fill_(float("nan"))
    out3 = eng.train_step(x, cls, gt, 100).clone()
    assert torch.equal(out1, out3) and torch.equal(g1, eng.grads)
    d1 = eng.forward(x, cls).clone()
    eng._work.view(torch.float32)[:] = float("nan")
    assert torch.equal(d1, eng.forward(x, cls))


def test_step_bits_equal_the_parent(built_lib):
    """Sharing the logits and parameter-gradient tiles with the segmentation head (csrc/dvt_head_dev.h) did not change a
    bit: one step and one forward at C 384, B 3, 9 x 11 tokens (one ragged slab per image, the B >= 3 gradient loss; with
    and without the SigLoss warm-up) and at C 768, B 2, 30 x 39 tokens (five slabs per image, 4 x 256 + 146) give the
    digests recorded from the parent commit on an MI355X (tests/golden/heads_parent.json; tools/record_head_golden.py
    wrote it)."""
    import hashlib
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heads_parent.json")) as f:
        want = json.load(f)["depth"]

    def digest(*ts):
        return hashlib.sha256(b"".join(t.detach().cpu().contiguous().numpy().tobytes() for t in ts)).hexdigest()
    for C, B, h, w, H, W, it in [(384, 3, 9, 11, 45, 61, 0), (384, 3, 9, 11, 45, 61, 100), (768, 2, 30, 39, 416, 544, 100)]:
        eng = make_head(C, seed=C + B)
        x, cls, gt = make_batch(B, h, w, C, H, W, seed=B + it)
        out = eng.train_step(x, cls, gt, it)
        got = {"step": digest(out, eng.grads), "forward": digest(eng.forward(x, cls))}
        assert got == want[f"C{C}_B{B}_{h}x{w}_it{it}"], f"depth head C {C} B {B} {h} x {w} it {it}: bits differ from the parent commit"


def test_forward_matches_reference(built_lib):
    eng = make_head(384, seed=2)
    x, cls, _ = make_batch(2, 9, 11, 384, 45, 61, seed=4)
    v = eng.views()
    want = ref.head(v["conv_depth.weight"].double().cpu(), v["conv_depth.bias"].double().cpu(), x.double().cpu(),
                    cls.double().cpu())[:, 0]
    got = eng.forward(x, cls)
    assert got.shape == (2, 36, 44) and rel(got, want) < 1e-5


# ---------------------------------------------------------------------------------------------------- optimiser
@pytest.mark.parametrize("scale", [1.0, 400.0])
def test_clip_grad_norm(built_lib, scale):
    eng = make_head(384, seed=3)
    g = torch.Generator().manual_seed(1)
    grads = torch.randn(eng.total, generator=g) * 0.01 * scale
    eng.grads.copy_(grads)
    W, b = grads[:eng.off_b].clone().requires_grad_(True), grads[eng.off_b:].clone().requires_grad_(True)
    W.grad, b.grad = W.detach().clone(), b.detach().clone()
    norm = torch.nn.utils.clip_grad_norm_([W, b], 35.0)
    assert (norm.item() > 35.0) == (scale > 1.0)
    out = eng.clip_grad_norm(35.0).cpu()
    assert abs(out[0].item() - norm.item()) <= 1e-5 * norm.item()
    assert rel(eng.grads, torch.cat([W.grad, b.grad])) < 1e-5
    if scale == 1.0:
        assert out[1].item() == 1.0 and torch.equal(eng.grads.cpu(), grads)


def test_five_adamw_steps_match_torch(built_lib):
    from dvt_amd.depth import cosine_lr, onecycle_beta1
    eng = make_head(384, seed=6)
    v = eng.views()
    W = v["conv_depth.weight"].double().cpu().clone().requires_grad_(True)
    b = v["conv_depth.bias"].double().cpu().clone().requires_grad_(True)
    opt = torch.optim.AdamW([W, b], lr=1.0, betas=(0.9, 0.999), weight_decay=0.01)
    max_iters, warm = 40, 10
    for i, it in enumerate((0, 5, 11, 12, 39)):
        x, cls, gt = make_batch(2, 9, 11, 384, 45, 61, seed=60 + i)
        lr = cosine_lr(it, 0.005, max_iters, warmup_iters=warm)
        beta1 = onecycle_beta1(it, max_iters)
        for gr in opt.param_groups:  # the groups rewritten every step, as mmcv's hooks do
            gr["lr"], gr["betas"] = lr, (beta1, 0.999)
        opt.zero_grad()
        ld, lg = ref.losses(W, b, x.double().cpu(), cls.double().cpu(), gt.double().cpu(), False)
        (ld + lg).backward()
        torch.nn.utils.clip_grad_norm_([W, b], 35.0)
        opt.step()
        eng.train_step(x, cls, gt, 100)
        eng.clip_grad_norm(35.0)
        eng.adamw_step(lr, 0.01, (beta1, 0.999))
    v = eng.views()
    errs = {"W": rel(v["conv_depth.weight"], W.detach()), "b": rel(v["conv_depth.bias"], b.detach())}
    print("five AdamW steps:", errs)
    assert max(errs.values()) < 1e-5, errs
    assert bool((eng.grads == 0).all()) and eng.step == 5


def test_state_dict_round_trip(built_lib):
    from dvt_amd.depth import DepthHeadEngine, state_dict_shapes
    eng = make_head(384, seed=8)
    sd = eng.state_dict()
    assert {k: tuple(t.shape) for k, t in sd.items()} == state_dict_shapes(384)
    assert sd["decode_head.conv_depth.weight"].shape == (256, 768, 1, 1)
    other = DepthHeadEngine(384, DEV, seed=99)
    other.load_state_dict(sd)
    assert torch.equal(other.params, eng.params)
    with pytest.raises(ValueError):
        other.load_state_dict({**sd, "decode_head.conv_depth.bias": torch.zeros(3)})


# ---------------------------------------------------------------------------------------------------- inference
def synthetic_maps(seed, flip=True, uh=120, uw=160, H=480, W=640):
    """Depth maps that leave [1e-3, 10] in places (the clamp acts), and a ground truth whose ratio to the prediction stays
    more than 1e-4 away from 1.25, 1.25^2 and 1.25^3 at every pixel."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, uh), torch.linspace(0, 1, uw), indexing="ij")
    d0 = 4.0 + 7.5 * torch.sin(3 * yy + 2 * xx) + 0.2 * torch.randn(uh, uw, generator=g)
    d1 = (4.0 + 7.5 * torch.sin(3 * yy + 2 * xx) + 0.2 * torch.randn(uh, uw, generator=g)).flip(-1)
    pred = ref.predict(d0, d1 if flip else None, (H, W))
    ratio = torch.exp(torch.randn(H, W, generator=g).double() * 0.4)
    for t in (1.25, 1.25 ** 2, 1.25 ** 3):
        for r in (t, 1.0 / t):
            near = (ratio / r - 1).abs() < 1e-3
            ratio[near] = r * 1.01
    gt = (pred * ratio).float()
    gt[torch.rand(H, W, generator=g) < 0.05] = 0.0
    return d0, d1, gt, pred


@pytest.mark.parametrize("flip", [True, False])
def test_inference_and_metrics(built_lib, flip):
    eng = make_head(384, seed=1)
    d0, d1, gt, want_pred = synthetic_maps(3, flip)
    want = np.array(ref.image_metrics(gt.numpy(), want_pred.numpy()))
    m = gt.numpy() > 0
    th = np.maximum(gt.double().numpy()[m] / want_pred.numpy()[m], want_pred.numpy()[m] / gt.double().numpy()[m])
    for t in (1.25, 1.25 ** 2, 1.25 ** 3):
        assert (np.abs(th / t - 1) > 1e-4).all()
    assert float(d0.min()) < 1e-3 and float(d0.max()) > 10.0  # the clamp acts
    row = torch.full((9,), -1.0, device=DEV, dtype=torch.float64)
    pred = eng.evaluate_maps(d0.to(DEV).contiguous(), d1.to(DEV).contiguous() if flip else None, gt.to(DEV), row, want_pred=True)
    assert rel(pred, want_pred) < 1e-5
    got = row.cpu().numpy()
    print("metrics", dict(zip(ref.METRICS, got)), "want", want)
    assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want)), (got, want)


def test_empty_mask_gives_nans_that_nanmean_skips(built_lib):
    from dvt_amd.depth import summarize
    eng = make_head(384, seed=1)
    d0, d1, gt, _ = synthetic_maps(4)
    table = torch.zeros(2, 9, device=DEV, dtype=torch.float64)
    eng.evaluate_maps(d0.to(DEV), d1.to(DEV), gt.to(DEV), table[0])
    empty = gt.clone()
    empty[45:471, 41:601] = 0.0  # valid pixels outside the Eigen crop only
    eng.evaluate_maps(d0.to(DEV), d1.to(DEV), empty.to(DEV), table[1])
    t = table.cpu().numpy()
    assert np.isnan(t[1]).all() and np.isfinite(t[0]).all()
    s = summarize(t)
    assert all(s[k] == t[0, i] for i, k in enumerate(ref.METRICS))


def test_evaluate_image_runs_the_flip_through_the_backbone(built_lib):
    from dvt_amd.depth import DepthHeadEngine
    from dvt_amd.seg import ViTBackbone
    from dvt_amd.vit import random_state_dict
    sd = random_state_dict(128, 2, 14, 1 + 16, seed=2, well_conditioned=True)
    # C = 128 is a multiple of 64: the head accepts it
    eng = DepthHeadEngine(128, DEV, seed=3)
    eng.views()["conv_depth.weight"].mul_(3.0)
    bb = ViTBackbone(sd, 14, DEV, dtype="float32", return_cls=True)
    g = torch.Generator().manual_seed(0)
    img = torch.randn(3, 60, 80, generator=g).to(DEV)
    gt = (0.5 + 8 * torch.rand(60, 80, generator=g)).to(DEV)
    row = torch.zeros(9, device=DEV, dtype=torch.float64)
    pred = eng.evaluate_image(img, gt, row, bb, crop=None, want_pred=True)
    f, c = bb(torch.stack([img, img.flip(-1)]))
    d = eng.forward(f, c)
    want_pred = ref.predict(d[0].cpu(), d[1].cpu(), (60, 80))
    assert rel(pred, want_pred) < 1e-5
    want = np.array(ref.image_metrics(gt.cpu().numpy(), want_pred.numpy(), crop=None))
    assert np.all(np.abs(row.cpu().numpy() - want) <= 1e-5 * np.abs(want))
