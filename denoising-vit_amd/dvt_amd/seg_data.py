"""Data side of the segmentation evaluation: the PascalVOC / ADE20K readers and mmseg 0.27's train and test pipelines of
the linear configs, restated with PIL and numpy (no cv2, mmcv or torchvision here), and a threaded feeder.

Random draws follow mmseg's transforms in order, from one numpy RandomState per sample seeded by (seed, rank, iteration,
position), so a resumed run draws what the uninterrupted run drew.  Not pinned to the reference: cv2's fixed-point
bilinear weights (PIL's bilinear filter is used) and cv2's uint8 HSV rounding (restated from the published formulas).
"""
from __future__ import annotations

import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

IMG_MEAN = np.array([123.675, 116.28, 103.53], np.float32)
IMG_STD = np.array([58.395, 57.12, 57.375], np.float32)
IGNORE = 255

VOC_CLASSES = ("background", "aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow",
               "diningtable", "dog", "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")
# the 150 SceneParsing categories, in the benchmark's published order
ADE_CLASSES = tuple("""wall building sky floor tree ceiling road bed windowpane grass cabinet sidewalk person earth door table
mountain plant curtain chair car water painting sofa shelf house sea mirror rug field armchair seat fence desk rock wardrobe
lamp bathtub railing cushion base box column signboard chest_of_drawers counter sand sink skyscraper fireplace refrigerator
grandstand path stairs runway case pool_table pillow screen_door stairway river bridge bookcase blind coffee_table toilet
flower book hill bench countertop stove palm kitchen_island computer swivel_chair boat bar arcade_machine hovel bus towel
light truck tower chandelier awning streetlight booth television_receiver airplane dirt_track apparel pole land bannister
escalator ottoman bottle buffet poster stage van ship fountain conveyer_belt canopy washer plaything swimming_pool stool
barrel basket waterfall tent bag minibike cradle oven ball food step tank trade_name microwave pot animal bicycle lake
dishwasher screen blanket sculpture hood sconce vase traffic_light tray ashcan fan pier crt_screen plate monitor
bulletin_board shower radiator glass clock flag""".split())
assert len(ADE_CLASSES) == 150


# ================================================================================================ datasets
class PascalVOCDataset:
    reduce_zero_label = False
    CLASSES = VOC_CLASSES

    def __init__(self, data_root: str, split: str = "train", img_dir: str = "JPEGImages",
                 ann_dir: str = "SegmentationClass", split_file: str | None = None):
        split_file = split_file or os.path.join("ImageSets", "Segmentation", f"{split}.txt")
        with open(os.path.join(data_root, split_file)) as f:
            names = [ln.strip() for ln in f if ln.strip()]
        self.samples = [(os.path.join(data_root, img_dir, n + ".jpg"), os.path.join(data_root, ann_dir, n + ".png"))
                        for n in names]

    def __len__(self):
        return len(self.samples)


class ADE20KDataset:
    reduce_zero_label = True
    CLASSES = ADE_CLASSES

    def __init__(self, data_root: str, split: str = "train", img_dir: str | None = None, ann_dir: str | None = None,
                 split_file: str | None = None):
        sub = "training" if split == "train" else "validation"
        img_dir = os.path.join(data_root, img_dir or os.path.join("images", sub))
        ann_dir = os.path.join(data_root, ann_dir or os.path.join("annotations", sub))
        names = sorted(f[:-4] for f in os.listdir(img_dir) if f.endswith(".jpg"))
        self.samples = [(os.path.join(img_dir, n + ".jpg"), os.path.join(ann_dir, n + ".png")) for n in names]

    def __len__(self):
        return len(self.samples)


DATASETS = {"PascalVOCDataset": PascalVOCDataset, "ADE20KDataset": ADE20KDataset}


def load_pair(ds, i: int):
    """-> (RGB uint8 [H, W, 3], label uint8 [H, W]); ADE20K's reduce_zero_label applied."""
    img_path, ann_path = ds.samples[i]
    img = np.asarray(Image.open(img_path).convert("RGB"), np.uint8)
    lab = np.array(Image.open(ann_path), np.uint8)
    if ds.reduce_zero_label:
        lab = reduce_zero_label(lab)
    return img, lab


def reduce_zero_label(lab: np.ndarray) -> np.ndarray:
    out = lab.astype(np.int16) - 1
    out[lab == 0] = IGNORE
    out[lab == IGNORE] = IGNORE
    return out.astype(np.uint8)


# ================================================================================================ transforms
def rescale_size(w: int, h: int, scale: tuple) -> tuple:
    """mmcv.rescale_size with a (long, short) edge bound: -> (new_w, new_h)."""
    f = min(max(scale) / max(h, w), min(scale) / min(h, w))
    return int(w * f + 0.5), int(h * f + 0.5)


def resize(img: np.ndarray, lab: np.ndarray | None, new_w: int, new_h: int):
    im = np.asarray(Image.fromarray(img).resize((new_w, new_h), Image.BILINEAR))
    lb = None if lab is None else np.asarray(Image.fromarray(lab).resize((new_w, new_h), Image.NEAREST))
    return im, lb


def crop_bbox(shape, crop, rng):
    mh, mw = max(shape[0] - crop[0], 0), max(shape[1] - crop[1], 0)
    y, x = rng.randint(0, mh + 1), rng.randint(0, mw + 1)
    return y, y + crop[0], x, x + crop[1]


def random_crop_bbox(lab: np.ndarray, crop, cat_max_ratio: float, rng):
    """mmseg RandomCrop: up to 10 re-draws until no class covers cat_max_ratio of the crop's non-ignored pixels."""
    box = crop_bbox(lab.shape, crop, rng)
    if cat_max_ratio < 1.0:
        for _ in range(10):
            y1, y2, x1, x2 = box
            labels, cnt = np.unique(lab[y1:y2, x1:x2], return_counts=True)
            cnt = cnt[labels != IGNORE]
            if len(cnt) > 1 and np.max(cnt) / np.sum(cnt) < cat_max_ratio:
                break
            box = crop_bbox(lab.shape, crop, rng)
    return box


def _convert(x, alpha=1.0, beta=0.0):
    return np.clip(x.astype(np.float32) * alpha + beta, 0, 255).astype(np.uint8)


def rgb_to_hsv(img: np.ndarray) -> np.ndarray:
    """uint8 HSV with H in [0, 180), S and V in [0, 255] (the OpenCV 8-bit convention)."""
    x = img.astype(np.float32)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    v = x.max(-1)
    mn = x.min(-1)
    d = v - mn
    s = np.where(v > 0, 255.0 * d / np.maximum(v, 1e-12), 0.0)
    dd = np.maximum(d, 1e-12)
    h = np.where(v == r, 60.0 * (g - b) / dd, np.where(v == g, 120.0 + 60.0 * (b - r) / dd, 240.0 + 60.0 * (r - g) / dd))
    h = np.where(d == 0, 0.0, h)
    h = np.where(h < 0, h + 360.0, h)
    out = np.stack([np.round(h / 2.0) % 180, np.round(s), v], -1)
    return out.astype(np.uint8)


def hsv_to_rgb(hsv: np.ndarray) -> np.ndarray:
    h = hsv[..., 0].astype(np.float32) * 2.0
    s = hsv[..., 1].astype(np.float32) / 255.0
    v = hsv[..., 2].astype(np.float32)
    c = v * s
    hp = (h / 60.0) % 6
    xx = c * (1 - np.abs(hp % 2 - 1))
    z = np.zeros_like(c)
    i = np.floor(hp).astype(np.int32)
    r = np.choose(i, [c, xx, z, z, xx, c])
    g = np.choose(i, [xx, c, c, xx, z, z])
    b = np.choose(i, [z, z, xx, c, c, xx])
    m = v - c
    return np.clip(np.round(np.stack([r + m, g + m, b + m], -1)), 0, 255).astype(np.uint8)


def photometric_distortion(img: np.ndarray, rng, brightness_delta=32, contrast=(0.5, 1.5), saturation=(0.5, 1.5),
                           hue_delta=18) -> np.ndarray:
    """mmseg PhotoMetricDistortion, draws in its order."""
    if rng.randint(2):
        img = _convert(img, beta=rng.uniform(-brightness_delta, brightness_delta))
    mode = rng.randint(2)
    if mode == 1 and rng.randint(2):
        img = _convert(img, alpha=rng.uniform(*contrast))
    if rng.randint(2):
        hsv = rgb_to_hsv(img)
        hsv[..., 1] = _convert(hsv[..., 1], alpha=rng.uniform(*saturation))
        img = hsv_to_rgb(hsv)
    if rng.randint(2):
        hsv = rgb_to_hsv(img)
        hsv[..., 0] = (hsv[..., 0].astype(int) + rng.randint(-hue_delta, hue_delta)) % 180
        img = hsv_to_rgb(hsv)
    if mode == 0 and rng.randint(2):
        img = _convert(img, alpha=rng.uniform(*contrast))
    return img


def normalize(img: np.ndarray) -> np.ndarray:
    return (img.astype(np.float32) - IMG_MEAN) / IMG_STD


def pad(img: np.ndarray, lab: np.ndarray, size):
    """mmseg Pad(size): bottom / right; image 0 (after Normalize), label 255."""
    H, W = size
    out = np.zeros((H, W, img.shape[2]), np.float32)
    out[:img.shape[0], :img.shape[1]] = img
    ol = np.full((H, W), IGNORE, np.uint8)
    ol[:lab.shape[0], :lab.shape[1]] = lab
    return out, ol


def train_sample(img, lab, rng, img_scale=(2048, 512), ratio_range=(0.5, 2.0), crop=(512, 512), cat_max_ratio=0.75,
                 flip_prob=0.5):
    """Resize (random ratio, keep ratio) -> RandomCrop -> RandomFlip -> PhotoMetricDistortion -> Normalize -> Pad.
    -> (CHW float32 normalised image, label)."""
    ratio = rng.random_sample() * (ratio_range[1] - ratio_range[0]) + ratio_range[0]
    scale = (int(img_scale[0] * ratio), int(img_scale[1] * ratio))
    nw, nh = rescale_size(img.shape[1], img.shape[0], scale)
    img, lab = resize(img, lab, nw, nh)
    y1, y2, x1, x2 = random_crop_bbox(lab, crop, cat_max_ratio, rng)
    img, lab = img[y1:y2, x1:x2], lab[y1:y2, x1:x2]
    if rng.rand() < flip_prob:
        img, lab = img[:, ::-1], lab[:, ::-1]
    img = photometric_distortion(np.ascontiguousarray(img), rng)
    img, lab = pad(normalize(img), np.ascontiguousarray(lab), crop)
    return np.ascontiguousarray(img.transpose(2, 0, 1)), lab


def test_sample(img, img_scale=(2048, 512)):
    """Keep-ratio Resize to img_scale, then Normalize: -> CHW float32."""
    nw, nh = rescale_size(img.shape[1], img.shape[0], img_scale)
    img, _ = resize(img, None, nw, nh)
    return np.ascontiguousarray(normalize(img).transpose(2, 0, 1))


# ================================================================================================ sampling and feeding
def epoch_order(n: int, epoch: int, seed: int, rank: int, world: int) -> np.ndarray:
    """DistributedSampler(shuffle=True): a permutation seeded by seed + epoch, padded to a multiple of world, rank's
    stride."""
    g = torch.Generator().manual_seed(seed + epoch)
    idx = torch.randperm(n, generator=g).tolist()
    total = -(-n // world) * world
    idx += idx[:total - n]
    return np.asarray(idx[rank:total:world])


def batch_indices(n: int, it: int, batch: int, seed: int, rank: int, world: int) -> list:
    """Dataset indices of iteration `it` on this rank (iterations run through the rank's epochs back to back; the last
    partial batch of an epoch is dropped, as mmseg's IterLoader with drop_last)."""
    per = -(-n // world)
    per_epoch = max(per // batch, 1)
    epoch, k = divmod(it, per_epoch)
    order = epoch_order(n, epoch, seed, rank, world)
    return [int(order[(k * batch + j) % len(order)]) for j in range(batch)]


class TrainFeeder:
    """Host thread pool (at most 16 workers) decoding and augmenting the batches of the next iterations into pinned
    buffers; `next()` -> (images [B, 3, crop] and labels [B, crop] on the device, host wait seconds)."""

    def __init__(self, ds, batch, crop, seed, rank, world, first_iter, last_iter, device, workers=8, depth=3, **aug):
        self.ds, self.batch, self.crop, self.seed, self.rank, self.world = ds, batch, tuple(crop), seed, rank, world
        self.device, self.aug = device, aug
        self.pool = ThreadPoolExecutor(max_workers=max(1, min(16, workers)))
        self.pending = queue.Queue()
        self.it, self.last = first_iter, last_iter
        self.lock = threading.Lock()
        for _ in range(depth):
            self._submit()

    def _load(self, it, j, index, img_buf, lab_buf):
        rng = np.random.RandomState([self.seed & 0xFFFFFFFF, self.rank, it, j])
        img, lab = load_pair(self.ds, index)
        im, lb = train_sample(img, lab, rng, crop=self.crop, **self.aug)
        img_buf[j].copy_(torch.from_numpy(im))
        lab_buf[j].copy_(torch.from_numpy(lb))

    def _submit(self):
        if self.it >= self.last:
            return
        it = self.it
        self.it += 1
        pin = torch.cuda.is_available()
        img_buf = torch.empty((self.batch, 3) + self.crop, dtype=torch.float32, pin_memory=pin)
        lab_buf = torch.empty((self.batch,) + self.crop, dtype=torch.uint8, pin_memory=pin)
        idx = batch_indices(len(self.ds), it, self.batch, self.seed, self.rank, self.world)
        futs = [self.pool.submit(self._load, it, j, i, img_buf, lab_buf) for j, i in enumerate(idx)]
        self.pending.put((futs, img_buf, lab_buf))

    def next(self):
        import time
        futs, img_buf, lab_buf = self.pending.get_nowait()
        t0 = time.perf_counter()
        for f in futs:
            f.result()
        wait = time.perf_counter() - t0
        self._submit()
        return (img_buf.to(self.device, non_blocking=True), lab_buf.to(self.device, non_blocking=True), wait)

    def close(self):
        self.pool.shutdown(wait=True, cancel_futures=True)
