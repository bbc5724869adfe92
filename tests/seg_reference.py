"""float64 restatement of the linear-probe segmentation evaluation (mmseg 0.27 BNHead + conv_seg + CrossEntropyLoss,
EncoderDecoder.slide_inference, intersect_and_union, total_area_to_metrics), written from the published semantics with
torch autograd as the reference for the HIP kernels of csrc/dvt_seg.hip."""
import numpy as np
import torch
import torch.nn.functional as F


def head_step(x, labels, W, b, gamma, beta, running_mean, running_var, momentum=0.1, eps=1e-5):
    """x [B, h, w, C], labels [B, H, W] (int, 255 ignored), W [K, C].  -> dict of loss, acc, gradients (float64) and the
    updated running statistics.  The loss is the CE summed over the valid pixels divided by ALL B H W pixels."""
    d = torch.float64
    x = x.to(d).permute(0, 3, 1, 2)
    params = [t.to(d).clone().requires_grad_(True) for t in (W, b, gamma, beta)]
    Wd, bd, gd, betad = params
    rm, rv = running_mean.to(d).clone(), running_var.to(d).clone()
    y = F.batch_norm(x, rm, rv, gd, betad, training=True, momentum=momentum, eps=eps)
    z = torch.einsum("bchw,kc->bkhw", y, Wd) + bd[None, :, None, None]
    up = F.interpolate(z, size=tuple(labels.shape[1:]), mode="bilinear", align_corners=False)
    lab = labels.long()
    loss = F.cross_entropy(up, lab, ignore_index=255, reduction="sum") / lab.numel()
    loss.backward()
    valid = lab != 255
    pred = up.argmax(1)
    eps32 = float(np.finfo(np.float32).eps)
    acc = ((pred == lab) & valid).sum().item() + eps32
    acc = acc * 100.0 / (valid.sum().item() + eps32)
    return {"loss": loss.item(), "acc": acc, "dW": Wd.grad, "db": bd.grad, "dgamma": gd.grad, "dbeta": betad.grad,
            "running_mean": rm, "running_var": rv, "z": z.permute(0, 2, 3, 1).detach()}


def head_forward(x, W, b, gamma, beta, running_mean, running_var, eps=1e-5):
    d = torch.float64
    y = (x.to(d) - running_mean.to(d)) / torch.sqrt(running_var.to(d) + eps) * gamma.to(d) + beta.to(d)
    return y @ W.to(d).T + b.to(d)


def slide_logits(crop_logits, boxes, H, W, out_size):
    """crop_logits: list of [h, w, K] per box (y1, y2, x1, x2); -> the resized seg logits [K, oh, ow] (float64)."""
    K = crop_logits[0].shape[-1]
    preds = torch.zeros(1, K, H, W, dtype=torch.float64)
    count = torch.zeros(1, 1, H, W, dtype=torch.float64)
    for z, (y1, y2, x1, x2) in zip(crop_logits, boxes):
        up = F.interpolate(z.to(torch.float64).permute(2, 0, 1)[None], size=(y2 - y1, x2 - x1), mode="bilinear",
                           align_corners=False)
        preds[:, :, y1:y2, x1:x2] += up
        count[:, :, y1:y2, x1:x2] += 1
    preds = preds / count
    return F.interpolate(preds, size=out_size, mode="bilinear", align_corners=False)[0]


def reduce_zero_label(label):
    label = np.asarray(label).astype(np.int64).copy()
    label[label == 0] = 255
    label = label - 1
    label[label == 254] = 255
    return label


def intersect_and_union(pred, label, K, ignore_index=255, reduce_zero=False):
    """mmseg 0.27 intersect_and_union restated in numpy: -> (area_intersect, area_union, area_pred, area_label)."""
    pred = np.asarray(pred).astype(np.int64)
    label = reduce_zero_label(label) if reduce_zero else np.asarray(label).astype(np.int64)
    mask = label != ignore_index
    pred, label = pred[mask], label[mask]
    inter = pred[pred == label]
    hist = lambda v: np.bincount(v[(v >= 0) & (v < K)], minlength=K)[:K]  # noqa: E731  (torch.histc over [0, K - 1])
    ai, ap, al = hist(inter), hist(pred), hist(label)
    return ai, ap + al - ai, ap, al


def metrics(total_inter, total_union, total_pred, total_label):
    ti, tu, tl = (np.asarray(v, np.float64) for v in (total_inter, total_union, total_label))
    with np.errstate(divide="ignore", invalid="ignore"):
        iou, acc = ti / tu, ti / tl
    return {"aAcc": ti.sum() / tl.sum(), "IoU": iou, "Acc": acc, "mIoU": np.nanmean(iou), "mAcc": np.nanmean(acc)}
