"""GPU: the linear-probe segmentation head and evaluation (csrc/dvt_seg.hip via dvt_amd.seg) against the float64
restatement in tests/seg_reference.py: the training step (loss, acc_seg, every parameter gradient, running statistics),
the statistics of channels with large means, determinism, AdamW with the poly schedule, and slide inference with the
intersect_and_union histograms."""
import numpy as np
import pytest
import torch

from tests import seg_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return ((got - want).norm() / want.norm()).item()


def make_head(C, K, seed):
    from dvt_amd.seg import SegHeadEngine
    eng = SegHeadEngine(C, K, DEV, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    v = eng.views()
    v["conv_seg.weight"].mul_(20.0)  # logits of order one: the softmax gradient is not trivially uniform
    v["conv_seg.bias"].copy_(torch.randn(K, generator=g) * 0.1)
    v["bn.weight"].copy_(1.0 + 0.2 * torch.randn(C, generator=g))
    v["bn.bias"].copy_(0.2 * torch.randn(C, generator=g))
    eng.running.copy_(torch.cat([torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)]))
    return eng


def make_batch(B, h, w, C, K, H, W, seed, all_ignore=False, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, h, w, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g) + mean
    lab = torch.randint(0, K, (B, H, W), generator=g, dtype=torch.int64).to(torch.uint8)
    lab[:, :3] = 255  # a 255 border, as Pad leaves it
    lab[:, :, W - 5:] = 255
    if all_ignore:
        lab[:] = 255
    return x.to(DEV).contiguous(), lab.to(DEV).contiguous()


def reference_step(eng, x, lab):
    v = {k: t.detach().cpu() for k, t in eng.views().items()}
    C = eng.C
    return ref.head_step(x.to(DEV), lab.to(DEV), v["conv_seg.weight"].to(DEV), v["conv_seg.bias"].to(DEV),
                         v["bn.weight"].to(DEV), v["bn.bias"].to(DEV), eng.running[:C].clone(), eng.running[C:].clone())


@pytest.mark.parametrize("C", [384, 768])
@pytest.mark.parametrize("K", [21, 150])
@pytest.mark.parametrize("B", [1, 3])
def test_head_step_matches_autograd(built_lib, C, K, B):
    h, w, H, W = 9, 11, 45, 61  # label size not a multiple of the feature grid
    eng = make_head(C, K, seed=C + K + B)
    x, lab = make_batch(B, h, w, C, K, H, W, seed=B)
    want = reference_step(eng, x, lab)
    out = eng.train_step(x, lab).cpu()
    torch.cuda.synchronize()
    g = eng.views(eng.grads)
    assert abs(out[0].item() - want["loss"]) <= 1e-5 * abs(want["loss"])
    assert abs(out[1].item() - want["acc"]) <= 1e-5 * abs(want["acc"])
    errs = {"dW": rel(g["conv_seg.weight"], want["dW"]), "db": rel(g["conv_seg.bias"], want["db"]),
            "dgamma": rel(g["bn.weight"], want["dgamma"]), "dbeta": rel(g["bn.bias"], want["dbeta"]),
            "running_mean": rel(eng.running[:C], want["running_mean"]),
            "running_var": rel(eng.running[C:], want["running_var"])}
    assert max(errs.values()) < 1e-5, errs
    assert eng.num_batches_tracked == 1


def test_head_step_at_the_training_geometry(built_lib):
    """samples_per_gpu 2, a 512 x 512 crop: 37 x 37 tokens after the centre padding to 518."""
    C, K, B = 768, 21, 2
    eng = make_head(C, K, seed=7)
    x, lab = make_batch(B, 37, 37, C, K, 512, 512, seed=11)
    want = reference_step(eng, x, lab)
    out = eng.train_step(x, lab).cpu()
    g = eng.views(eng.grads)
    assert abs(out[0].item() - want["loss"]) <= 1e-5 * abs(want["loss"])
    assert abs(out[1].item() - want["acc"]) <= 1e-5 * abs(want["acc"])
    for name, key in (("conv_seg.weight", "dW"), ("conv_seg.bias", "db"), ("bn.weight", "dgamma"), ("bn.bias", "dbeta")):
        assert rel(g[name], want[key]) < 1e-5, name


def test_head_step_all_ignored(built_lib):
    C, K = 384, 21
    eng = make_head(C, K, seed=3)
    x, lab = make_batch(2, 9, 11, C, K, 45, 61, seed=5, all_ignore=True)
    out = eng.train_step(x, lab).cpu()
    assert out[0].item() == 0.0
    assert out[1].item() == pytest.approx(float(np.finfo(np.float32).eps) * 100 / float(np.finfo(np.float32).eps))
    assert torch.count_nonzero(eng.grads).item() == 0


def test_statistics_keep_the_variance_of_large_means(built_lib):
    C, K = 768, 21
    eng = make_head(C, K, seed=9)
    g = torch.Generator().manual_seed(0)
    x = (1e3 + torch.randn(4, 37, 37, C, generator=g)).to(DEV)
    st = eng.batch_stats(x).cpu().double()
    xd = x.double().reshape(-1, C)
    n = xd.shape[0]
    assert st[3 * C].item() == n
    assert rel(st[:C] + st[C:2 * C], xd.mean(0)) < 1e-12
    assert rel(st[2 * C:3 * C] / n, xd.var(0, unbiased=False)) < 1e-5
    # merging two halves (SyncBN over two ranks) gives the whole batch's record
    halves = torch.stack([eng.batch_stats(x[:2].contiguous()), eng.batch_stats(x[2:].contiguous())])
    merged = eng.merge_stats(halves).cpu().double()
    assert rel(merged[2 * C:3 * C] / n, xd.var(0, unbiased=False)) < 1e-5
    assert merged[3 * C].item() == n
    # and the step on such features still matches autograd
    lab = torch.randint(0, K, (4, 61, 61), generator=g).to(torch.uint8).to(DEV)
    small = x[:, :9, :9].contiguous()
    lab = lab[:, :45, :45].contiguous()
    want = reference_step(eng, small, lab)
    out = eng.train_step(small, lab).cpu()
    assert abs(out[0].item() - want["loss"]) <= 1e-5 * abs(want["loss"])
    assert rel(eng.views(eng.grads)["conv_seg.weight"], want["dW"]) < 1e-5


def test_deterministic_and_nan_workspace(built_lib):
    C, K = 768, 150
    x, lab = make_batch(3, 37, 37, C, K, 300, 400, seed=2)
    runs = []
    for fill in (None, None, float("nan")):
        eng = make_head(C, K, seed=1)
        if fill is not None:
            eng._work = torch.empty(1 << 30, device=DEV, dtype=torch.uint8)
            eng._work.view(torch.float32).fill_(fill)
        out = eng.train_step(x, lab).clone()
        runs.append((out.cpu(), eng.grads.cpu(), eng.running.cpu()))
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)


def test_step_bits_equal_the_parent(built_lib):
    """Sharing the logits and parameter-gradient tiles with the depth head (csrc/dvt_head_dev.h) did not change a bit: one
    step and one forward at C 384, K 21 / 150, B 3, 9 x 11 tokens (297 rows: five row tiles with a ragged last one, slabs of
    256 + 41 rows; one partial class tile / three with a ragged third) give the digests recorded from the parent commit on
    an MI355X (tests/golden/heads_parent.json; tools/record_head_golden.py wrote it)."""
    import hashlib
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heads_parent.json")) as f:
        want = json.load(f)["seg"]

    def digest(*ts):
        return hashlib.sha256(b"".join(t.detach().cpu().contiguous().numpy().tobytes() for t in ts)).hexdigest()
    C = 384
    for K in (21, 150):
        eng = make_head(C, K, seed=C + K)
        x, lab = make_batch(3, 9, 11, C, K, 45, 61, seed=3)
        out = eng.train_step(x, lab)
        got = {"step": digest(out, eng.grads, eng.running), "forward": digest(eng.forward(x))}
        assert got == want[f"C{C}_K{K}"], f"seg head C {C} K {K}: bits differ from the parent commit"


def test_adamw_five_steps_with_poly_schedule(built_lib):
    from dvt_amd.seg import poly_lr
    C, K = 384, 21
    eng = make_head(C, K, seed=4)
    names = ["conv_seg.weight", "conv_seg.bias", "bn.weight", "bn.bias"]
    tparams = [eng.views()[n].detach().clone().requires_grad_(True) for n in names]
    opt = torch.optim.AdamW(tparams, lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.999))
    for it in range(5):
        lr = poly_lr(it, 1e-3, 10, warmup_iters=3)
        x, lab = make_batch(2, 9, 11, C, K, 45, 61, seed=20 + it)
        eng.train_step(x, lab)
        grads = eng.views(eng.grads)
        for p, n in zip(tparams, names):
            p.grad = grads[n].detach().clone()
        for group in opt.param_groups:
            group["lr"] = lr
        opt.step()
        eng.adamw_step(lr, 1e-4)
        for p, n in zip(tparams, names):
            assert rel(eng.views()[n], p.detach()) < 1e-5, (it, n)
    assert torch.count_nonzero(eng.grads).item() == 0


class _Backbone:
    """A fixed, smooth stand-in for the ViT: patch-average of the image projected to C channels, on the 14-pixel grid of
    the centre-padded crop."""

    def __init__(self, C, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.P = (torch.randn(3, C, generator=g) * 2).to(DEV)
        self.Q = (torch.randn(3, C, generator=g)).to(DEV)

    def __call__(self, crops):
        from dvt_amd.seg import center_pad
        _, _, H, W = crops.shape
        (t, b), (l, r) = center_pad(H, 14), center_pad(W, 14)
        x = torch.nn.functional.pad(crops, (l, r, t, b))
        f = torch.nn.functional.avg_pool2d(x, 14).permute(0, 2, 3, 1)
        return (torch.tanh(f @ self.P) + f @ self.Q).contiguous()


@pytest.mark.parametrize("C,K,reduce_zero", [(768, 21, False), (384, 150, True)])
def test_slide_inference_and_histograms(built_lib, C, K, reduce_zero):
    from dvt_amd.seg import slide_windows
    eng = make_head(C, K, seed=5)
    bb = _Backbone(C, seed=1)
    g = torch.Generator().manual_seed(3)
    H, W, oh, ow = 512, 683, 375, 500
    img = torch.nn.functional.interpolate(torch.randn(1, 3, 24, 32, generator=g), size=(H, W), mode="bilinear")[0]
    img = img.to(DEV).contiguous()
    label = torch.randint(0, K + 1 if reduce_zero else K, (oh, ow), generator=g).to(torch.uint8)
    label[:4] = 255
    label = label.to(DEV).contiguous()
    canvas, count = eng.slide_inference(img, bb)
    boxes = slide_windows(H, W)
    assert len(boxes) == 2
    v = {k: t.detach() for k, t in eng.views().items()}
    crop_logits = []
    for (y1, y2, x1, x2) in boxes:
        f = bb(img[None, :, y1:y2, x1:x2].contiguous())[0]
        crop_logits.append(ref.head_forward(f, v["conv_seg.weight"], v["conv_seg.bias"], v["bn.weight"], v["bn.bias"],
                                            eng.running[:C], eng.running[C:]).cpu())
    want = ref.slide_logits(crop_logits, boxes, H, W, (oh, ow))
    # the canvas before the final resize
    want_canvas = ref.slide_logits(crop_logits, boxes, H, W, (H, W))
    assert rel((canvas / count).cpu(), want_canvas) < 1e-5
    hist = torch.zeros(3, K, dtype=torch.int64, device=DEV)
    pred = eng.finalize(canvas, count, (oh, ow), label, hist, reduce_zero_label=reduce_zero, want_pred=True).cpu()
    top2 = want.topk(2, dim=0).values
    near_tie = (top2[0] - top2[1]) < 1e-4 * top2[0].abs().clamp(min=1.0)
    ref_pred = want.argmax(0)
    mismatch = pred.long() != ref_pred
    assert not (mismatch & ~near_tie).any()
    ai, au, ap, al = ref.intersect_and_union(pred.numpy(), label.cpu().numpy(), K, reduce_zero=reduce_zero)
    got = hist.cpu().numpy()
    np.testing.assert_array_equal(got, np.stack([ai, ap, al]))  # exact, on the kernel's own argmax
    ri, _, rp, rl = ref.intersect_and_union(ref_pred.numpy(), label.cpu().numpy(), K, reduce_zero=reduce_zero)
    ties = int(near_tie.sum())
    assert np.abs(got - np.stack([ri, rp, rl])).sum() <= 4 * ties  # against the float64 argmax, up to near ties
    # a second image accumulates into the same histogram
    eng.finalize(canvas, count, (oh, ow), label, hist, reduce_zero_label=reduce_zero)
    np.testing.assert_array_equal(hist.cpu().numpy(), 2 * got)
