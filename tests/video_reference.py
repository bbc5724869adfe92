"""Float64 / numpy / PIL restatement of the per-frame lines of the reference's make_video_demo.py (115-217), of Pillow's
8-bit bicubic resize, and a query-chunked fp32 ViT forward for sequences whose S x S logits do not fit (oracle/vit.py
materialises them).  Test reference only: nothing in dvt_amd imports it.

Everything that the script computes in the features' precision is float64 here; the uint8 pictures are formed as the script
forms them (`(v * 255).astype(np.uint8)` after a matplotlib colour map where it uses one).
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

MAP_KINDS = ("pca_instance", "pca_dataset", "kmeans", "first_pca", "second_pca", "third_pca", "fg_pca", "fg_pca_standard",
             "norm")


# ================================================================================================ Pillow's bicubic, 8 bit
def _keys(x: np.ndarray) -> np.ndarray:
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def _resample_axis(img: np.ndarray, out_size: int) -> np.ndarray:
    """One pass along axis 0 of a uint8 array [in, ...]."""
    in_size = img.shape[0]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    out = np.empty((out_size,) + img.shape[1:], np.uint8)
    src = img.astype(np.int64)
    for i in range(out_size):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        k = _keys((np.arange(xmin, xmax) - center + 0.5) * (1.0 / filterscale))
        ww = 0.0
        for w in k:  # the sum in Pillow's order
            ww += w
        if ww != 0.0:
            k = k / ww
        ki = np.where(k < 0, np.trunc(-0.5 + k * (1 << 22)), np.trunc(0.5 + k * (1 << 22))).astype(np.int64)
        acc = (1 << 21) + np.tensordot(ki, src[xmin:xmax], axes=(0, 0))
        out[i] = np.clip(acc >> 22, 0, 255).astype(np.uint8)
    return out


def bicubic_resize_u8(img: np.ndarray, out_hw) -> np.ndarray:
    """uint8 [h, w, c] -> uint8 [H, W, c] as `Image.fromarray(img).resize((W, H), Image.BICUBIC)`: the horizontal pass first,
    into a uint8 intermediate, then the vertical one."""
    H, W = int(out_hw[0]), int(out_hw[1])
    hor = _resample_axis(np.ascontiguousarray(img.transpose(1, 0, 2)), W).transpose(1, 0, 2)
    return _resample_axis(np.ascontiguousarray(hor), H)


def apply_tables_u8(img: np.ndarray, xb, xc, yb, yc) -> np.ndarray:
    """The resize from GIVEN (bounds, coefficients) tables, as csrc/dvt_video.hip's k_resample does it."""
    def one(a, bounds, coef):
        out = np.empty((bounds.shape[0],) + a.shape[1:], np.uint8)
        src = a.astype(np.int64)
        for i, (first, cnt) in enumerate(bounds):
            acc = (1 << 21) + np.tensordot(coef[i, :cnt].astype(np.int64), src[first:first + cnt], axes=(0, 0))
            out[i] = np.clip(acc >> 22, 0, 255).astype(np.uint8)
        return out
    hor = one(np.ascontiguousarray(img.transpose(1, 0, 2)), xb, xc).transpose(1, 0, 2)
    return one(np.ascontiguousarray(hor), yb, yc)


# ================================================================================================ the per-frame lines
def kmeans_predict(x: np.ndarray, centers: np.ndarray):
    """Cosine assignment (largest similarity, lowest index on a tie, a zero vector has similarity 0) -> (labels, gap between
    the two largest similarities of every row)."""
    x, c = x.astype(np.float64), centers.astype(np.float64)
    den = np.linalg.norm(x, axis=1)[:, None] * np.linalg.norm(c, axis=1)[None]
    sim = np.divide(x @ c.T, den, out=np.zeros_like(den), where=den > 0)
    labels = sim.argmax(1)
    if sim.shape[1] > 1:
        top = np.sort(sim, axis=1)
        gap = top[:, -1] - top[:, -2]
    else:
        gap = np.full(sim.shape[0], np.inf)
    return labels, gap


def _minmax(v):
    return (v - v.min(0, keepdims=True)) / (v.max(0, keepdims=True) - v.min(0, keepdims=True))


def _cmap_u8(name, v):
    import matplotlib
    return (matplotlib.colormaps[name](v)[..., :3] * 255).astype(np.uint8)


def frame_values(x, instance, dataset, standard, fg, fg_standard, centers) -> dict:
    """Float64 values of one frame before any picture is formed.  x [n, C]; bases [C, 3] ([C, 1] for `standard`)."""
    x = np.asarray(x, np.float64)
    v = {"pca_instance": x @ instance.astype(np.float64), "pca_full": x @ dataset.astype(np.float64),
         "standard": (x @ standard.astype(np.float64))[:, 0], "fg": x @ fg.astype(np.float64),
         "fg_standard": x @ fg_standard.astype(np.float64), "norms": np.linalg.norm(x, axis=1)}
    v["labels"], v["label_gap"] = kmeans_predict(x, centers)
    v["second"] = 1 - v["pca_full"][:, 1]
    v["mask_fg"] = v["second"] > 0.1
    v["mask_standard"] = v["standard"] > 0
    t = v["norms"] / 5
    p = np.exp(t - t.max())
    p = p / p.sum()
    v["norm_map"] = (p - p.min()) / (p.max() - p.min())
    return v


def frame_unit_maps(v: dict) -> dict:
    """kind -> the float64 values in [0, 1] that the script multiplies by 255 (colour maps: the scalar fed to the map)."""
    return {"pca_instance": _minmax(v["pca_instance"]), "pca_dataset": _minmax(v["pca_full"]),
            "first_pca": _minmax(v["pca_full"][:, 0]), "second_pca": _minmax(v["second"]),
            "third_pca": _minmax(v["pca_full"][:, 2]),
            "fg_pca": _minmax(v["fg"]) * v["mask_fg"][:, None], "fg_pca_standard": _minmax(v["fg_standard"]) * v["mask_standard"][:, None],
            "norm": v["norm_map"]}


def frame_token_pictures(v: dict, grid_hw, num_clusters: int = 8) -> dict:
    """kind -> uint8 [h, w, 3], the nine token-resolution pictures of the script from the values of `frame_values`."""
    h, w = grid_hw
    u = frame_unit_maps(v)
    out = {}
    for kind in ("pca_instance", "pca_dataset", "fg_pca", "fg_pca_standard"):
        out[kind] = (u[kind].reshape(h, w, 3) * 255).astype(np.uint8)
    for kind in ("first_pca", "second_pca", "third_pca", "norm"):
        out[kind] = _cmap_u8("inferno", u[kind].reshape(h, w))
    out["kmeans"] = _cmap_u8("rainbow", v["labels"].astype(np.float32).reshape(h, w) / num_clusters)
    return out


def input_picture(img_normalised: torch.Tensor, mean, std) -> np.ndarray:
    """Lines 90-92: the denormalised, clamped, truncated input picture, uint8 [H, W, 3] (fp32 tensor arithmetic)."""
    m = torch.tensor([-a / b for a, b in zip(mean, std)], dtype=torch.float32).view(3, 1, 1)
    s = torch.tensor([1 / b for b in std], dtype=torch.float32).view(3, 1, 1)
    img = (img_normalised.float().reshape(3, *img_normalised.shape[-2:]) - m) / s
    return (img.permute(1, 2, 0).clamp(0, 1).numpy() * 255).astype(np.uint8)


# ================================================================================================ long-sequence ViT
def chunked_vit_forward(sd: dict, img: torch.Tensor, patch: int, stride: int, q_chunk: int = 768, eps: float = 1e-6):
    """oracle.vit.forward_features in fp32 with the attention evaluated `q_chunk` queries at a time (all heads): at most
    heads x q_chunk x S logits live at once (12 x 768 x 25 321 x 4 B = 0.93 GB at the demo shape).  Every query row still
    sees all keys in one softmax, so this is the same arithmetic up to the order of the matrix products' sums."""
    from oracle.vit import resample_abs_pos_embed
    dim = sd["pos_embed"].shape[-1]
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    heads = dim // 64
    with torch.no_grad():
        x = F.conv2d(img, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=stride)
        B, _, gh, gw = x.shape
        x = x.permute(0, 2, 3, 1).reshape(B, gh * gw, dim)
        n_reg = sd["reg_token"].shape[1] if "reg_token" in sd else 0
        pos = resample_abs_pos_embed(sd["pos_embed"], (gh, gw), num_prefix_tokens=0 if n_reg else 1)
        if n_reg:
            x = torch.cat([sd["cls_token"].expand(B, -1, -1), sd["reg_token"].expand(B, -1, -1), x + pos], dim=1)
        else:
            x = torch.cat([sd["cls_token"].expand(B, -1, -1), x], dim=1) + pos
        S = x.shape[1]
        for i in range(depth):
            p = f"blocks.{i}."
            h = F.layer_norm(x, (dim,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
            qkv = F.linear(h, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
            qkv = qkv.reshape(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
            q, k, v = qkv.unbind(0)
            kt = k.transpose(-2, -1).contiguous()
            a = torch.empty(B, heads, S, 64)
            for s0 in range(0, S, q_chunk):
                a[:, :, s0:s0 + q_chunk] = torch.softmax((q[:, :, s0:s0 + q_chunk] * 64 ** -0.5) @ kt, dim=-1) @ v
            a = a.transpose(1, 2).reshape(B, S, dim)
            a = F.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
            x = x + sd.get(p + "ls1.gamma", 1.0) * a
            h = F.layer_norm(x, (dim,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
            h = F.linear(F.gelu(F.linear(h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])),
                         sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
            x = x + sd.get(p + "ls2.gamma", 1.0) * h
        x = F.layer_norm(x, (dim,), sd["norm.weight"], sd["norm.bias"], eps)
        return x[:, 1 + n_reg:].reshape(B, gh, gw, dim)


def q_chunk_for(heads: int, n_tokens: int, budget_bytes: int = 1 << 30) -> int:
    """Queries per chunk so that heads x chunk x n_tokens fp32 logits stay below `budget_bytes`."""
    return max(1, budget_bytes // (4 * heads * n_tokens))


def seeded_feature_map(shape, seed: int) -> np.ndarray:
    """A float32 map [h, w, C] at the scale of final-normed ViT tokens (channels O(1), row norms of a few tens, as the
    softmax(|x| / 5) of the script presumes): smooth components with a decaying spectrum over noise."""
    h, w, c = shape
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    comps = np.stack([np.sin(3 * xx + yy), np.cos(2 * yy - xx), xx * yy, np.sin(5 * yy)], -1)
    x = comps @ (rng.standard_normal((4, c)) * np.array([1.2, 0.7, 0.4, 0.25])[:, None]) + 0.5 * rng.standard_normal((h, w, c))
    x = x + 0.3 * rng.standard_normal(c)
    return (x * (40.0 / math.sqrt(c)) / np.sqrt((x ** 2).mean())).astype(np.float32)
