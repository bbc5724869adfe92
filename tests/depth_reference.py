"""Float64 restatement of the depth probe, written from the semantics of the reference's evaluation/depth (its BNHead
without a norm layer, SigLoss, GradientLoss, DepthEncoderDecoder's test path and core/evaluation/metrics.py), with torch
autograd.  The head upsamples FIRST and convolves afterwards, as the reference does, so the kernels' commuted order is
checked against the un-commuted definition."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3
METRICS = ("a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel")


def head(weight, bias, feats, cls, n_bins=256, min_depth=1e-3, max_depth=10.0, upsample=4):
    """weight [K, 2C], bias [K], feats NHWC [B, h, w, C], cls [B, C] -> depth [B, 1, up h, up w]."""
    B, h, w, C = feats.shape
    x = feats.permute(0, 3, 1, 2)
    x = torch.cat([x, cls[:, :, None, None].expand(B, C, h, w)], 1)
    x = F.interpolate(x, scale_factor=upsample, mode="bilinear", align_corners=False)
    z = F.conv2d(x, weight[:, :, None, None], bias)
    p = torch.relu(z) + 0.1
    p = p / p.sum(1, keepdim=True)
    bins = torch.linspace(min_depth, max_depth, n_bins, dtype=weight.dtype)
    return (p * bins[None, :, None, None]).sum(1, keepdim=True)


def sig_loss(pred, gt, warm_up):
    m = gt > 0
    g = torch.log(pred[m] + EPS) - torch.log(gt[m] + EPS)
    if warm_up:
        return torch.sqrt(0.15 * torch.mean(g) ** 2)
    return torch.sqrt(torch.var(g) + 0.15 * torch.mean(g) ** 2)


def gradient_loss(pred, gt):
    """GradientLoss as its indexing computes it on [B, 1, H, W] tensors: the sub-sampling and the differences run over the
    batch and channel axes.  A sub-sampled batch without a valid pixel contributes 0 (the reference: 0 / 0 with a zero
    gradient)."""
    total = pred.new_zeros(())
    for s in (None, 2, 4, 6):
        a, t = (pred, gt) if s is None else (pred[::s, ::s], gt[::s, ::s])
        mask = t > 0
        N = mask.sum()
        d = (torch.log(a + EPS) - torch.log(t + EPS)) * mask
        v = torch.abs(d[0:-2, :] - d[2:, :]) * (mask[0:-2, :] * mask[2:, :])
        hgrad = torch.abs(d[:, 0:-2] - d[:, 2:]) * (mask[:, 0:-2] * mask[:, 2:])
        if N > 0:
            total = total + (hgrad.sum() + v.sum()) / N
    return total


def losses(weight, bias, feats, cls, gt, warm_up, **kw):
    """-> (loss_depth, 0.5 * gradient loss); gt [B, H, W], 0 = invalid."""
    d = head(weight, bias, feats, cls, **kw)
    d = F.interpolate(d, size=gt.shape[1:], mode="bilinear", align_corners=False)
    return sig_loss(d, gt[:, None], warm_up), 0.5 * gradient_loss(d, gt[:, None])


def step_reference(weight, bias, feats, cls, gt, warm_up, **kw):
    """Float64 autograd of one step: -> loss_depth, loss_grad, dW [K, 2C], db [K]."""
    W = weight.double().clone().requires_grad_(True)
    b = bias.double().clone().requires_grad_(True)
    ld, lg = losses(W, b, feats.double(), cls.double(), gt.double(), warm_up, **kw)
    (ld + lg).backward()
    return float(ld.detach()), float(lg.detach()), W.grad, b.grad


def clip_factor(grads, max_norm):
    norm = torch.sqrt(sum((g.double() ** 2).sum() for g in grads))
    return float(norm), float(min(1.0, max_norm / (float(norm) + 1e-6)))


def resize_to(d, size):
    return F.interpolate(d[None, None], size=size, mode="bilinear", align_corners=False)[0, 0]


def predict(d0, d1, size, min_depth=1e-3, max_depth=10.0):
    """The test path from the head's depth maps of an image (d0) and of its horizontal flip (d1 or None)."""
    out = resize_to(d0.double().clamp(min_depth, max_depth), size)
    if d1 is not None:
        out = (out + resize_to(d1.double().clamp(min_depth, max_depth), size).flip(-1)) / 2
    return out


def calculate(gt, pred):
    if gt.shape[0] == 0:
        return (np.nan,) * 9
    thresh = np.maximum(gt / pred, pred / gt)
    a1, a2, a3 = (thresh < 1.25).mean(), (thresh < 1.25 ** 2).mean(), (thresh < 1.25 ** 3).mean()
    abs_rel = np.mean(np.abs(gt - pred) / gt)
    sq_rel = np.mean((gt - pred) ** 2 / gt)
    rmse = np.sqrt(((gt - pred) ** 2).mean())
    rmse_log = np.sqrt(((np.log(gt) - np.log(pred)) ** 2).mean())
    err = np.log(pred) - np.log(gt)
    with np.errstate(invalid="ignore"):
        silog = np.sqrt(np.mean(err ** 2) - np.mean(err) ** 2) * 100
    if np.isnan(silog):
        silog = 0
    log_10 = np.abs(np.log10(gt) - np.log10(pred)).mean()
    return a1, a2, a3, abs_rel, rmse, log_10, rmse_log, silog, sq_rel


def image_metrics(gt, pred, min_depth=1e-3, max_depth=10.0, crop=(45, 471, 41, 601)):
    """pre_eval of one image: gt, pred [H, W] numpy -> the nine metrics."""
    gt, pred = np.asarray(gt, np.float64), np.asarray(pred, np.float64)
    mask = np.logical_and(gt > min_depth, gt < max_depth)
    if crop is not None:
        inside = np.zeros_like(mask)
        inside[crop[0]:crop[1], crop[2]:crop[3]] = True
        mask = np.logical_and(mask, inside)
    return calculate(gt[mask], pred[mask])


def train_reference(sample_fn, weight, bias, n_iters, lr_fn, beta1_fn, weight_decay=0.01, max_norm=35.0, **kw):
    """The training loop in float64 with torch.optim.AdamW: sample_fn(it) -> (feats, cls, gt)."""
    W = weight.double().clone().requires_grad_(True)
    b = bias.double().clone().requires_grad_(True)
    opt = torch.optim.AdamW([W, b], lr=1.0, betas=(0.9, 0.999), weight_decay=weight_decay)
    for it in range(n_iters):
        feats, cls, gt = sample_fn(it)
        for gr in opt.param_groups:
            gr["lr"], gr["betas"] = lr_fn(it), (beta1_fn(it), 0.999)
        opt.zero_grad()
        if not bool((gt > 0).any()):
            continue
        ld, lg = losses(W, b, feats.double(), cls.double(), gt.double(), it < 100, **kw)
        (ld + lg).backward()
        torch.nn.utils.clip_grad_norm_([W, b], max_norm)
        opt.step()
    return W.detach(), b.detach()
