"""Float64 CPU reference of the visualisation kernels (include/dvt_vis.h), written for the tests.

Plain numpy / torch, no product code: the PCA basis by `eigh` of the covariance, the robust colour range by sorting,
Lloyd's cosine k-means step by step, resampling through `torch.nn.functional.interpolate` in float64, and the colour-table
rule.  Conventions (tie rules, which assignment the labels belong to) are those of the header.
"""
from __future__ import annotations

import numpy as np
import torch


# ------------------------------------------------------------------------------------------------ PCA
def pca_basis(x, mask=None):
    """(basis [C, 3], eigenvalues [3]) of the selected rows: eigh of sum (x - mean)(x - mean)^T / (count - 1), leading
    three, each with its largest-magnitude component (lowest index on a tie) positive."""
    x = np.asarray(x, np.float64).reshape(-1, np.shape(x)[-1])
    if mask is not None:
        x = x[np.asarray(mask).reshape(-1) != 0]
    xc = x - x.mean(axis=0, keepdims=True)
    cov = xc.T @ xc / (x.shape[0] - 1)
    w, v = np.linalg.eigh(cov)
    order = np.argsort(w)[::-1][:3]
    basis = v[:, order].copy()
    for j in range(3):
        if basis[np.argmax(np.abs(basis[:, j])), j] < 0:
            basis[:, j] = -basis[:, j]
    return basis, w[order]


def one_minus_abs_cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - np.abs((a * b).sum(0)) / (np.linalg.norm(a, axis=0) * np.linalg.norm(b, axis=0))


def lower_median_row(v, rows):
    """(value, row) of torch's median of v[rows]: the lower middle value; the lowest row among equal values."""
    vals = v[rows]
    order = np.argsort(vals, kind="stable")
    val = vals[order[(len(rows) - 1) // 2]]
    return val, int(rows[np.nonzero(vals == val)[0][0]])


def robust_range(colors, mask=None, m=2.0):
    """get_robust_pca's range from projected rows [n, 3], in float64.  Returns a dict: rgb_min / rgb_max [3], median /
    deviation [3], rows int [13] (median, deviation, min, max rows per channel, then the fall-back flag)."""
    colors = np.asarray(colors, np.float64).reshape(-1, 3)
    n = colors.shape[0]
    rows = np.arange(n) if mask is None else np.nonzero(np.asarray(mask).reshape(-1) != 0)[0]
    out = {"rgb_min": np.full(3, np.nan), "rgb_max": np.full(3, np.nan), "median": np.full(3, np.nan),
           "deviation": np.full(3, np.nan), "rows": np.full(13, -1, np.int64)}
    out["rows"][12] = 0
    if len(rows) == 0:
        return out
    fallback = False
    for c in range(3):
        v = colors[:, c]
        med, r_med = lower_median_row(v, rows)
        d = np.abs(v - med)
        dev, r_dev = lower_median_row(d, rows)
        out["median"][c], out["deviation"][c] = med, dev
        out["rows"][c], out["rows"][3 + c] = r_med, r_dev
        with np.errstate(divide="ignore", invalid="ignore"):
            inl = rows[(d[rows] / dev) < m]
        if len(inl) == 0:
            fallback = True
            continue
        lo, hi = v[inl].min(), v[inl].max()
        out["rgb_min"][c], out["rgb_max"][c] = lo, hi
        out["rows"][6 + c] = int(inl[np.nonzero(v[inl] == lo)[0][0]])
        out["rows"][9 + c] = int(inl[np.nonzero(v[inl] == hi)[0][0]])
    if fallback:  # the reference's except branch: the extremes over ALL rows and all three channels
        lo, hi = colors.min(), colors.max()
        r_lo = r_hi = -1  # the row of the first CHANNEL that holds the extreme, as the kernel reports it
        for c in range(3):
            if (colors[:, c] == lo).any():
                r_lo = int(np.nonzero(colors[:, c] == lo)[0][0])
                break
        for c in range(3):
            if (colors[:, c] == hi).any():
                r_hi = int(np.nonzero(colors[:, c] == hi)[0][0])
                break
        out["rgb_min"][:], out["rgb_max"][:] = lo, hi
        out["rows"][6:9], out["rows"][9:12], out["rows"][12] = r_lo, r_hi, 1
    return out


def fg_mask(colors, thresh=0.2):
    """(mask, value): value = (colors[:, 0] - min) / (max - min) over all rows, mask = value < thresh: the foreground rows of
    get_robust_pca(remove_first_component=True)."""
    c0 = np.asarray(colors, np.float64).reshape(-1, 3)[:, 0]
    v = (c0 - c0.min()) / (c0.max() - c0.min())
    return v < thresh, v


def robust_pca(x, m=2.0, basis=None, mask=None):
    """(basis, rgb_min, rgb_max) with the basis given or from pca_basis; the UN-centred rows are projected."""
    x = np.asarray(x, np.float64).reshape(-1, np.shape(x)[-1])
    if basis is None:
        basis, _ = pca_basis(x, mask)
    r = robust_range(x @ np.asarray(basis, np.float64), mask, m)
    return np.asarray(basis, np.float64), r["rgb_min"], r["rgb_max"]


def pca_colors(x, basis, rgb_min, rgb_max):
    """clamp((x basis - min) / (max - min), 0, 1), shape of x with 3 channels."""
    x = np.asarray(x, np.float64)
    c = x @ np.asarray(basis, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (c - np.asarray(rgb_min, np.float64)) / (np.asarray(rgb_max, np.float64) - np.asarray(rgb_min, np.float64))
    return np.clip(c, 0.0, 1.0)


# ------------------------------------------------------------------------------------------------ scalar maps
def scale_map(x):
    """[h, w, C] -> [h, w]: (|x| - min) / (max - min + 1e-6)."""
    nrm = np.linalg.norm(np.asarray(x, np.float64), axis=-1)
    return (nrm - nrm.min()) / (nrm.max() - nrm.min() + 1e-6)


def similarity_map(x):
    """[h, w, C] -> [h, w]: cosine with the centre row, min-max normalised, centre -1."""
    x = np.asarray(x, np.float64)
    h, w, _ = x.shape
    unit = x / np.linalg.norm(x, axis=-1, keepdims=True)
    sim = unit @ unit[h // 2, w // 2]
    sim = (sim - sim.min()) / (sim.max() - sim.min())
    sim[h // 2, w // 2] = -1.0
    return sim


# ------------------------------------------------------------------------------------------------ k-means
def kmeans_similarity(x, centers):
    x, centers = np.asarray(x, np.float64), np.asarray(centers, np.float64)
    den = np.linalg.norm(x, axis=1)[:, None] * np.linalg.norm(centers, axis=1)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, (x @ centers.T) / den, 0.0)


def kmeans_step(x, centers, labels=None):
    """One Lloyd iteration from `centers`: dict(labels, centers, inertia, shift, margin) -- margin [n] = the gap between the
    two largest similarities of each row.  `labels` given: the update uses THEM (the lock-step test assigns near-ties as
    the kernel did)."""
    x, centers = np.asarray(x, np.float64), np.asarray(centers, np.float64)
    sim = kmeans_similarity(x, centers)
    lab = np.argmax(sim, axis=1)  # (the first maximum: the lowest index on a tie)
    top = np.sort(sim, axis=1)
    margin = top[:, -1] - top[:, -2] if sim.shape[1] > 1 else np.full(len(x), np.inf)
    inertia = float((1.0 - sim[np.arange(len(x)), lab]).sum())
    use = lab if labels is None else np.asarray(labels)
    new = centers.copy()
    for k in range(centers.shape[0]):
        sel = use == k
        if sel.any():
            new[k] = x[sel].mean(axis=0)
    return {"labels": lab, "centers": new, "inertia": inertia, "shift": float(((new - centers) ** 2).sum()), "margin": margin}


def kmeans(x, init_centers, max_iter=100, tol=1e-4):
    """Restarts from init_centers [R, K, C]: labels / inertia of the LAST assignment, centres = the means of those labels."""
    runs = []
    for c0 in np.asarray(init_centers, np.float64):
        cen, it, st = c0, 0, None
        while it < max_iter:
            st = kmeans_step(x, cen)
            cen, it = st["centers"], it + 1
            if st["shift"] < tol:
                break
        runs.append({"labels": st["labels"], "centers": cen, "inertia": st["inertia"], "iterations": it})
    best = int(np.argmin([r["inertia"] for r in runs]))
    return {"best": best, "labels": runs[best]["labels"], "centers": runs[best]["centers"],
            "inertia": np.array([r["inertia"] for r in runs]), "iterations": np.array([r["iterations"] for r in runs])}


# ------------------------------------------------------------------------------------------------ rendering
def resample(a, size, interp="nearest"):
    """[h, w] or [h, w, c] -> [H, W(, c)] through torch.nn.functional.interpolate in float64."""
    t = torch.as_tensor(np.asarray(a, np.float64))
    squeeze = t.dim() == 2
    t = t[..., None] if squeeze else t
    kw = {"align_corners": False} if interp == "bilinear" else {}
    out = torch.nn.functional.interpolate(t.permute(2, 0, 1)[None], size=tuple(size), mode=interp, **kw)[0].permute(1, 2, 0)
    return (out[..., 0] if squeeze else out).numpy()


def table_index(v):
    """matplotlib's rule for a 256-entry map: min(int(clamp(v, 0, 1) * 256), 255)."""
    return np.minimum((np.clip(np.asarray(v, np.float64), 0.0, 1.0) * 256).astype(np.int64), 255)


def apply_table(v, table):
    return np.asarray(table, np.float64)[table_index(v)]


def scalar_panel(smap, size, table, interp="nearest", neg_red=False):
    v = resample(smap, size, interp)
    rgb = apply_table(v, table)
    if neg_red:
        rgb[v < 0] = (1.0, 0.0, 0.0)
    return rgb


def labels_panel(labels, size, table):
    lab = resample(np.asarray(labels, np.float64), size, "nearest").astype(np.int64)
    return np.asarray(table, np.float64)[lab]


def to_u8(rgb):
    """(uint8) (rgb * 255) with the canvas' float32 product."""
    return (np.clip(np.asarray(rgb, np.float32), 0, 1) * np.float32(255)).astype(np.uint8)
