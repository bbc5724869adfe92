"""Data side of the depth evaluation: the NYU Depth v2 reader and the train / test pipelines of the reference's
vitb_nyu_linear_config.py, restated with PIL and numpy (no cv2 or mmcv here), and the threaded feeder.

Random draws follow the reference's transforms in order, from one numpy RandomState per sample seeded by (seed, rank,
iteration, position), so a resumed run draws what the uninterrupted run drew.  Images are kept in RGB here; the reference
loads B, G, R, so ColorAug's three colour factors go to channels 2, 1, 0.  Restated, not checked against mmcv here:
`mmcv.imrotate` (cv2.warpAffine about ((w - 1) / 2, (h - 1) / 2), bilinear for the image, nearest for the depth, border 0).
"""
from __future__ import annotations

import os

import numpy as np
import torch
from PIL import Image

from .seg_data import IMG_MEAN, IMG_STD, TrainFeeder, batch_indices

NYU_CROP = (45, 472, 43, 608)  # NYUCrop: rows [45, 472), columns [43, 608)


# ================================================================================================ dataset
def parse_split(text: str, data_root: str) -> list:
    """Lines `image depth ...` relative to data_root (a leading slash removed); lines whose depth is `None` are dropped;
    -> [(image path, depth path)] sorted by the image path."""
    out = []
    for line in text.splitlines():
        parts = line.strip().split(" ")
        if len(parts) < 2 or parts[1] == "None":
            continue
        strip = lambda p: p[1:] if p.startswith("/") else p  # noqa: E731
        out.append((os.path.join(data_root, strip(parts[0])), os.path.join(data_root, strip(parts[1]))))
    return sorted(out, key=lambda s: s[0])


class NYUDataset:
    def __init__(self, data_root: str, split: str, depth_scale: float = 1000.0):
        path = split if os.path.isabs(split) else os.path.join(data_root, split)
        with open(path) as f:
            self.samples = parse_split(f.read(), data_root)
        self.depth_scale = float(depth_scale)

    def __len__(self):
        return len(self.samples)


def load_pair(ds: NYUDataset, i: int):
    """-> (image uint8 [H, W, 3] RGB, depth float32 [H, W] in metres, 0 = invalid)."""
    img_path, depth_path = ds.samples[i]
    img = np.asarray(Image.open(img_path).convert("RGB"))
    depth = np.asarray(Image.open(depth_path), dtype=np.float32) / ds.depth_scale
    return img, depth


# ================================================================================================ transforms
def nyu_crop(img, depth):
    y0, y1, x0, x1 = NYU_CROP
    return img[y0:y1, x0:x1], depth[y0:y1, x0:x1]


def rotate(arr: np.ndarray, angle: float, nearest: bool) -> np.ndarray:
    """mmcv.imrotate(arr, angle) (positive = clockwise), same size, border 0."""
    h, w = arr.shape[:2]
    cx, cy = (w - 1) * 0.5, (h - 1) * 0.5
    a = np.deg2rad(-angle)
    al, be = np.cos(a), np.sin(a)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    sx = al * (xs - cx) - be * (ys - cy) + cx
    sy = be * (xs - cx) + al * (ys - cy) + cy
    src = arr.astype(np.float64)

    def at(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
        return v * (ok[..., None] if v.ndim == 3 else ok)

    if nearest:
        return at(np.floor(sy + 0.5).astype(np.int64), np.floor(sx + 0.5).astype(np.int64)).astype(arr.dtype)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    fx, fy = sx - x0, sy - y0
    if arr.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    out = (at(y0, x0) * (1 - fx) + at(y0, x0 + 1) * fx) * (1 - fy) + (at(y0 + 1, x0) * (1 - fx) + at(y0 + 1, x0 + 1) * fx) * fy
    if arr.dtype == np.uint8:
        return np.clip(np.rint(out), 0, 255).astype(np.uint8)
    return out.astype(arr.dtype)


def random_rotate(img, depth, rng, prob=0.5, degree=2.5):
    """One rand() for the decision and one uniform(-degree, degree) ALWAYS drawn."""
    do = rng.rand() < prob
    angle = rng.uniform(-degree, degree)
    if do:
        img, depth = rotate(img, angle, nearest=False), rotate(depth, angle, nearest=True)
    return img, depth


def random_flip(img, depth, rng, prob=0.5):
    if rng.rand() < prob:
        img, depth = img[:, ::-1], depth[:, ::-1]
    return img, depth


def random_crop(img, depth, rng, crop=(416, 544)):
    """randint for y, then x."""
    mh, mw = max(img.shape[0] - crop[0], 0), max(img.shape[1] - crop[1], 0)
    oy = rng.randint(0, mh + 1)
    ox = rng.randint(0, mw + 1)
    return img[oy:oy + crop[0], ox:ox + crop[1]], depth[oy:oy + crop[0], ox:ox + crop[1]]


def color_aug(img: np.ndarray, rng, prob=0.5, gamma_range=(0.9, 1.1), brightness_range=(0.75, 1.25), color_range=(0.9, 1.1)):
    """On the 0-255 values: image ** gamma, times brightness, times three colour factors in the reference's B, G, R channel
    order, clipped to [0, 255].  -> float64 when applied, the input otherwise."""
    if not rng.rand() < prob:
        return img
    gamma = rng.uniform(*gamma_range)
    out = img.astype(np.float64) ** gamma
    out = out * rng.uniform(*brightness_range)
    colors = rng.uniform(color_range[0], color_range[1], size=3)
    out = out * colors[::-1][None, None, :]  # RGB here: colors[0] is blue's
    return np.clip(out, 0, 255)


def normalize(img: np.ndarray) -> np.ndarray:
    return ((img.astype(np.float32) - IMG_MEAN) / IMG_STD).astype(np.float32)


def train_sample(img, depth, rng, crop=(416, 544)):
    """NYUCrop -> RandomRotate -> RandomFlip -> RandomCrop -> ColorAug -> Normalize: (CHW float32, depth float32 [crop])."""
    img, depth = nyu_crop(img, depth)
    img, depth = random_rotate(img, depth, rng)
    img, depth = random_flip(img, depth, rng)
    img, depth = random_crop(img, depth, rng, crop)
    img = color_aug(np.ascontiguousarray(img), rng)
    return np.ascontiguousarray(normalize(img).transpose(2, 0, 1)), np.ascontiguousarray(depth, dtype=np.float32)


def test_sample(img):
    """The whole image, normalised: CHW float32 (the flip is taken on the device)."""
    return np.ascontiguousarray(normalize(img).transpose(2, 0, 1))


# ================================================================================================ feeding
class DepthTrainFeeder(TrainFeeder):
    """seg_data.TrainFeeder with the depth pipeline: `next()` -> (images [B, 3, crop], depth [B, crop] fp32, wait)."""

    def _load(self, it, j, index, img_buf, lab_buf):
        rng = np.random.RandomState([self.seed & 0xFFFFFFFF, self.rank, it, j])
        img, depth = load_pair(self.ds, index)
        im, dp = train_sample(img, depth, rng, crop=self.crop)
        img_buf[j].copy_(torch.from_numpy(im))
        lab_buf[j].copy_(torch.from_numpy(dp))

    def _submit(self):
        if self.it >= self.last:
            return
        it = self.it
        self.it += 1
        pin = torch.cuda.is_available()
        img_buf = torch.empty((self.batch, 3) + self.crop, dtype=torch.float32, pin_memory=pin)
        lab_buf = torch.empty((self.batch,) + self.crop, dtype=torch.float32, pin_memory=pin)
        idx = batch_indices(len(self.ds), it, self.batch, self.seed, self.rank, self.world)
        futs = [self.pool.submit(self._load, it, j, i, img_buf, lab_buf) for j, i in enumerate(idx)]
        self.pending.put((futs, img_buf, lab_buf))

    def next(self):
        """-> (images, depth, host wait seconds, whether the batch has a valid pixel -- read from the host buffer, so the
        driver can skip a step without reading the loss back)."""
        import time
        futs, img_buf, lab_buf = self.pending.get_nowait()
        t0 = time.perf_counter()
        for f in futs:
            f.result()
        wait = time.perf_counter() - t0
        self._submit()
        valid = bool((lab_buf > 0).any())
        return img_buf.to(self.device, non_blocking=True), lab_buf.to(self.device, non_blocking=True), wait, valid
