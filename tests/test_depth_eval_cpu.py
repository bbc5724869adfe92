"""CPU: the host pieces of the depth probe (dvt_amd.depth): the cosine / warm-up learning rate, the one-cycle beta1, the
summary of the metric table, the checkpoint names -- and the float64 restatement in tests/depth_reference.py itself:
the metrics against hand-computed values and what the reference's GradientLoss really computes over the batch axis."""
import math

import numpy as np
import pytest
import torch

from tests import depth_reference as ref


def test_cosine_lr_with_linear_warmup():
    from dvt_amd.depth import cosine_lr
    T, base = 38400, 0.005
    cos = lambda it: base * 1e-8 + 0.5 * (base - base * 1e-8) * (math.cos(math.pi * it / T) + 1)  # noqa: E731
    assert cosine_lr(0, base, T) == pytest.approx(cos(0) * 0.001, rel=1e-12)  # warmup_ratio at iteration 0
    k = (1 - 12799 / 12800) * (1 - 0.001)
    assert cosine_lr(12799, base, T) == pytest.approx(cos(12799) * (1 - k), rel=1e-12)
    assert cosine_lr(12800, base, T) == pytest.approx(cos(12800), rel=1e-12)  # the warm-up has ended
    assert cosine_lr(12800, base, T) == pytest.approx(0.5 * base * (math.cos(math.pi / 3) + 1), rel=1e-6)
    assert cosine_lr(38399, base, T) == pytest.approx(cos(38399), rel=1e-12)
    assert cosine_lr(38399, base, T) < 1e-8 * 2
    lrs = [cosine_lr(i, base, T) for i in range(0, T, 100)]
    peak = int(np.argmax(lrs))
    assert all(a < b for a, b in zip(lrs[:peak], lrs[1:peak + 1])) and all(a > b for a, b in zip(lrs[peak:], lrs[peak + 1:]))


def test_onecycle_beta1():
    from dvt_amd.depth import onecycle_beta1
    T = 38400
    assert onecycle_beta1(0, T) == pytest.approx(0.95, abs=1e-15)
    assert onecycle_beta1(int(0.3 * T) - 1, T) == pytest.approx(0.85, abs=1e-12)  # the end of the first phase
    assert onecycle_beta1(T - 1, T) == pytest.approx(0.95, abs=1e-12)
    mid = (int(0.3 * T) - 1) / 2
    assert onecycle_beta1(int(mid), T) == pytest.approx(0.90, abs=1e-4)
    b = [onecycle_beta1(i, T) for i in range(T)]
    assert min(b) >= 0.85 - 1e-12 and max(b) <= 0.95 + 1e-12 and int(np.argmin(b)) == int(0.3 * T) - 1


def test_summarize_is_a_nanmean_per_metric():
    from dvt_amd.depth import METRICS, summarize
    assert METRICS == ref.METRICS
    t = np.arange(27, dtype=np.float64).reshape(3, 9)
    t[1] = np.nan
    s = summarize(t)
    assert s["a1"] == 9.0 and s["sq_rel"] == 17.0
    assert all(math.isnan(v) for v in summarize(np.full((2, 9), np.nan)).values())


def test_state_dict_names():
    from dvt_amd.depth import state_dict_shapes
    assert state_dict_shapes(768) == {"decode_head.conv_depth.weight": (256, 1536, 1, 1),
                                      "decode_head.conv_depth.bias": (256,)}


def test_head_engine_needs_a_gpu():
    from dvt_amd import _lib
    from dvt_amd.depth import DepthHeadEngine
    with pytest.raises(_lib.DvtError):
        DepthHeadEngine(768, "cpu")


def test_library_declares_the_depth_and_cls_entry_points(built_lib):
    for name in ("dvt_depth_train_step", "dvt_depth_forward", "dvt_depth_clip_grad_norm", "dvt_depth_eval_image",
                 "dvt_vit_forward_cls", "dvt_vit_forward_f32_cls", "dvt_vit_forward_f32x3_cls"):
        assert hasattr(built_lib, name)
    out = (__import__("ctypes").c_int64 * 3)()
    assert built_lib.dvt_depth_param_offsets(768, 256, out) == 0 and list(out) == [0, 256 * 1536, 256 * 1536 + 256]
    assert built_lib.dvt_depth_param_offsets(100, 256, out) == -1
    assert built_lib.dvt_depth_workspace_bytes(2, 30, 39, 768, 256, 4, 416, 544) > 0
    assert built_lib.dvt_depth_workspace_bytes(65, 30, 39, 768, 256, 4, 416, 544) == -1
    assert built_lib.dvt_depth_workspace_bytes(2, 30, 39, 768, 256, 9, 416, 544) == -1


def test_metrics_against_hand_computed_values():
    gt = np.array([[2.0, 4.0, 0.0, 20.0]])
    pred = np.array([[2.0, 2.0, 5.0, 5.0]])
    a1, a2, a3, abs_rel, rmse, log_10, rmse_log, silog, sq_rel = ref.image_metrics(gt, pred, crop=None)
    # valid: (2, 2) and (4, 2); 0 and 20 fall outside (1e-3, 10)
    assert (a1, a2, a3) == (0.5, 0.5, 0.5)  # ratios 1 and 2, and 2 > 1.25^3 = 1.953125
    assert abs_rel == pytest.approx(0.25) and sq_rel == pytest.approx(0.5) and rmse == pytest.approx(math.sqrt(2.0))
    assert log_10 == pytest.approx(math.log10(2) / 2) and rmse_log == pytest.approx(math.log(2) / math.sqrt(2))
    assert silog == pytest.approx(100 * math.sqrt(math.log(2) ** 2 / 2 - (math.log(2) / 2) ** 2))
    assert all(math.isnan(v) for v in ref.image_metrics(np.zeros((2, 2)), np.ones((2, 2)), crop=None))
    # the Eigen crop is part of the mask
    big_gt, big_pred = np.full((480, 640), 2.0), np.full((480, 640), 2.0)
    big_pred[:45] = 4.0
    assert ref.image_metrics(big_gt, big_pred)[3] == 0.0 and ref.image_metrics(big_gt, big_pred, crop=None)[3] > 0


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5])
def test_gradient_loss_runs_over_the_batch_axis(B):
    g = torch.Generator().manual_seed(B)
    pred = (0.5 + torch.rand(B, 1, 6, 7, generator=g, dtype=torch.float64)).requires_grad_(True)
    gt = 0.5 + torch.rand(B, 1, 6, 7, generator=g, dtype=torch.float64)
    loss = ref.gradient_loss(pred, gt)
    if B <= 2:
        assert float(loss.detach()) == 0.0
        return
    assert float(loss) > 0.0
    # by hand: image j against image j + 2 of the batch sub-sampled by 1, 2, 4, 6
    d = torch.log(pred.detach() + 1e-3) - torch.log(gt + 1e-3)
    want = 0.0
    for s in (1, 2, 4, 6):
        idx = list(range(0, B, s))
        pairs = sum(float((d[idx[j]] - d[idx[j + 2]]).abs().sum()) for j in range(len(idx) - 2))
        want += pairs / (len(idx) * 42)
    assert float(loss) == pytest.approx(want, rel=1e-12)
    # shuffling the pixels of every image the same way leaves it unchanged: nothing in it is spatial
    perm = torch.randperm(42, generator=g)
    shuf = lambda t: t.reshape(B, 1, 42)[:, :, perm].reshape(B, 1, 6, 7)  # noqa: E731
    assert float(ref.gradient_loss(shuf(pred.detach()), shuf(gt))) == pytest.approx(float(loss), rel=1e-12)


def test_sig_loss_warm_up_and_variance():
    g = torch.Generator().manual_seed(0)
    pred = 0.5 + torch.rand(2, 1, 5, 5, generator=g, dtype=torch.float64)
    gt = 0.5 + torch.rand(2, 1, 5, 5, generator=g, dtype=torch.float64)
    gt[0, 0, 0] = 0.0
    m = gt > 0
    gg = (torch.log(pred + 1e-3) - torch.log(gt + 1e-3))[m].numpy()
    assert float(ref.sig_loss(pred, gt, True)) == pytest.approx(math.sqrt(0.15) * abs(gg.mean()), rel=1e-12)
    assert float(ref.sig_loss(pred, gt, False)) == pytest.approx(math.sqrt(gg.var(ddof=1) + 0.15 * gg.mean() ** 2), rel=1e-12)


def test_head_commutes_with_the_upsample():
    """What the kernels rely on: convolving the upsampled features equals upsampling the token logits."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(1)
    W = torch.randn(16, 2 * 8, generator=g, dtype=torch.float64)
    b = torch.randn(16, generator=g, dtype=torch.float64)
    x = torch.randn(2, 3, 5, 8, generator=g, dtype=torch.float64)
    cls = torch.randn(2, 8, generator=g, dtype=torch.float64)
    want = ref.head(W, b, x, cls, n_bins=16)
    z = torch.einsum("bhwc,kc->bkhw", x, W[:, :8]) + (cls @ W[:, 8:].T + b)[:, :, None, None]
    z = F.interpolate(z, scale_factor=4, mode="bilinear", align_corners=False)
    p = torch.relu(z) + 0.1
    got = (p / p.sum(1, keepdim=True) * torch.linspace(1e-3, 10, 16, dtype=torch.float64)[None, :, None, None]).sum(1, keepdim=True)
    assert float((got - want).abs().max()) < 1e-12
