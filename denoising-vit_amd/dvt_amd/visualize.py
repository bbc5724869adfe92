"""Pictures of what stage 1 has ALREADY written: no ViT, no fit.

    python -m dvt_amd.visualize --save_root out/ --model vit_base_patch14_dinov2.lvd142m --output_dir vis/ \\
        [--data_root data/ --img_path list.txt]

walks the `raw_features/<model>/**.npy` / `denoised_features/<model>/**.npy` pairs under --save_root (the layout of
`misc.output_paths`) and writes one labelled row per image: the input image (when --data_root is given and the image is
found), then PCA colours, k-means clusters, L2-norm map and centre-patch similarity of the raw and of the denoised features.
Each row is composed on the device by the kernels of `dvt_amd.vis` and leaves it in one copy; the previous picture is
encoded and written by a worker thread meanwhile.  Ranks of a torch.distributed.run launch take contiguous shards of the
pair list (`misc.shard_range`), as stage 1 does.
"""
from __future__ import annotations

import argparse
import glob
import os
import queue
import threading
import time

import numpy as np
import torch

from . import dist as D
from .utils import misc
from .utils import visualization as VZ
from .vis import VisEngine

IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".JPEG", ".png", ".bmp")


def get_args(argv=None):
    p = argparse.ArgumentParser(description="Visualise saved stage-1 features (MI355X)")
    p.add_argument("--save_root", type=str, required=True, help="stage 1's --save_root")
    p.add_argument("--model", type=str, default="vit_base_patch14_dinov2.lvd142m")
    p.add_argument("--data_root", type=str, default=None, help="stage 1's --data_root: adds the input image as first column")
    p.add_argument("--img_path", type=str, default=None, help="stage 1's work-list (.txt): image names with their extensions")
    p.add_argument("--output_dir", type=str, default="./work_dirs/visualization")
    p.add_argument("--panel_size", type=int, default=518, help="side of every panel in pixels")
    p.add_argument("--num_clusters", type=int, default=5)
    p.add_argument("--start_idx", type=int, default=0)
    p.add_argument("--num_imgs", type=int, default=100)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--vis_font", type=str, default=None, help="TrueType / OpenType file for the labels")
    return p.parse_args(argv)


# ---------------------------------------------------------------------------------------------------- pure host pieces
def find_pairs(save_root: str, model: str) -> list:
    """[(key, raw .npy, denoised .npy)], sorted by key = the path below raw_features/<model>/ without its extension; a raw
    file without its denoised twin is no pair."""
    raw_dir = os.path.join(save_root, "raw_features", model)
    den_dir = os.path.join(save_root, "denoised_features", model)
    out = []
    for raw_p in glob.glob(os.path.join(raw_dir, "**", "*.npy"), recursive=True):
        rel = os.path.relpath(raw_p, raw_dir)
        den_p = os.path.join(den_dir, rel)
        if os.path.isfile(den_p):
            out.append((os.path.splitext(rel)[0].replace(os.sep, "/"), raw_p, den_p))
    return sorted(out)


def select(pairs: list, start_idx: int, num_imgs: int) -> list:
    return pairs[start_idx: start_idx + num_imgs]


def shard(pairs: list, rank: int, world: int) -> list:
    lo, hi = misc.shard_range(0, len(pairs), rank, world)
    return pairs[lo:hi]


def image_lookup(data_root: str | None, img_path: str | None) -> dict:
    """key -> image file, from stage 1's work-list (first word of each line, below data_root)."""
    out = {}
    if data_root is None or img_path is None or not os.path.isfile(img_path):
        return out
    with open(img_path) as f:
        for line in f.read().splitlines():
            name = line.strip().split(" ")[0]
            if name:
                out[os.path.splitext(os.path.normpath(name))[0].replace(os.sep, "/")] = os.path.join(data_root, name)
    return out


def find_image(key: str, data_root: str | None, lookup: dict) -> str | None:
    if data_root is None:
        return None
    if key in lookup:
        return lookup[key] if os.path.isfile(lookup[key]) else None
    for ext in IMAGE_EXTENSIONS:
        cand = os.path.join(data_root, key + ext)
        if os.path.isfile(cand):
            return cand
    return None


def load_image(path: str) -> torch.Tensor:
    """float [3, H, W] in [0, 1] (host; resized to the panel on the device)."""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im.convert("RGB"), dtype=np.float32) / 255.0
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))


# ---------------------------------------------------------------------------------------------------- the sweep
def main(args, rank: int = 0, world: int = 1, device=None) -> int:
    from .vit import require_consumer_width
    require_consumer_width(args.model, "visualisation (DVT_VIS_MAX_C)")
    if device is None:
        device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(device)
    pairs = shard(select(find_pairs(args.save_root, args.model), args.start_idx, args.num_imgs), rank, world)
    lookup = image_lookup(args.data_root, args.img_path)
    os.makedirs(args.output_dir, exist_ok=True)
    hw = (args.panel_size, args.panel_size)
    eng = None
    writes: queue.Queue = queue.Queue(maxsize=2)
    errors = []

    def writer():
        while True:
            item = writes.get()
            if item is None:
                return
            try:
                host, event, path = item
                event.synchronize()
                VZ.save_image(path, host.numpy())
            except BaseException as e:  # noqa: BLE001 - re-raised by the sweep
                errors.append(e)

    th = threading.Thread(target=writer, name="dvt-vis-writer", daemon=True)
    th.start()
    start = time.time()
    done = 0
    try:
        for i, (key, raw_p, den_p) in enumerate(pairs):
            if errors:
                break
            raw = torch.from_numpy(np.load(raw_p)).to(device)
            den = torch.from_numpy(np.load(den_p)).to(device)
            raw = raw.reshape(-1, *raw.shape[-3:])[0]
            den = den.reshape(-1, *den.shape[-3:])[0]
            if eng is None:
                eng = VisEngine(device, max_rows=raw.shape[0] * raw.shape[1], max_channels=raw.shape[2],
                                max_clusters=max(args.num_clusters, 1))
            img_p = find_image(key, args.data_root, lookup)
            image = load_image(img_p) if img_p is not None else None
            tile, _ = VZ.compose_feature_row(eng, raw, den, hw, image, args.num_clusters, args.seed + args.start_idx + i,
                                             args.vis_font)
            host = torch.empty(tile.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(tile, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
            writes.put((host, event, os.path.join(args.output_dir, key + ".png")))
            done += 1
    finally:
        writes.put(None)
        th.join()
    if errors:
        raise errors[0]
    print(f"[rank {rank}] {done} pictures in {time.time() - start:.1f}s -> {args.output_dir}")
    return done


if __name__ == "__main__":
    a = get_args()
    r, w, _ = D.env_ranks()
    main(a, r, w)
