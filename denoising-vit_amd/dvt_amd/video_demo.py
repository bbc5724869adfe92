"""The feature-video demo: the reference's `make_video_demo.py` on the HIP extractor and the kernels of `dvt_amd.video`.

    python -m dvt_amd.video_demo --frames demo/davis-mallard-water --output_dir work_dirs/davis_demo --stats stats.npz \\
        [--vit_checkpoint ckpts/imgnet_distilled/vit_base_patch14_dinov2.lvd142m.pth | --allow_random_vit]

For every scene directory (frames sorted by name) and every frame i it writes `<output_dir>/<scene>/images/{i:02d}_<kind>.png`
for the ten kinds of the script (input, pca_instance, pca_dataset, kmeans, first_pca, second_pca, third_pca, fg_pca,
fg_pca_standard, norm) and one animation per kind, named as the script names its videos: `.mp4` through imageio when it
imports, otherwise an animated `.gif` through PIL.  The PCA bases, k-means centres and foreground bases are fitted on frame
0 of a scene and applied to all of its frames.  The finished pictures of a frame leave the device in one copy; a worker
thread encodes them while the next frame is computed.  As in the script, the pictures of a scene stay in host memory until its
animations are written (10 x frames x 1.25 MB at 490 x 854).
"""
from __future__ import annotations

import argparse
import os
import queue
import threading
import time

import numpy as np
import torch

from . import _lib
from . import video as VD
from . import vit as _vit

IMAGENET_MEAN, IMAGENET_STD = _vit.IMAGENET_MEAN, _vit.IMAGENET_STD
model_statistics = _vit.model_statistics


def get_args(argv=None):
    p = argparse.ArgumentParser(description="Feature-video demo (MI355X)")
    p.add_argument("--frames", type=str, action="append", required=True, help="a scene: a directory of frames (repeatable)")
    p.add_argument("--output_dir", type=str, default="work_dirs/davis_demo/")
    p.add_argument("--stats", type=str, required=True, help="the reference's demo/assets/stats.pth, or an .npz with its arrays")
    p.add_argument("--stats_prefix", type=str, default="denoised", choices=("denoised", "dinov2"))
    p.add_argument("--model", type=str, default="vit_base_patch14_dinov2.lvd142m")
    p.add_argument("--vit_checkpoint", type=str, default=None, help="a stage-3 *_distilled checkpoint or a timm state dict")
    p.add_argument("--allow_random_vit", action="store_true", help="random ViT weights (machines without a checkpoint)")
    p.add_argument("--height", type=int, default=490)
    p.add_argument("--width", type=int, default=854)
    p.add_argument("--stride_size", type=int, default=4)
    p.add_argument("--dtype", type=str, default="bfloat16", choices=("bfloat16", "float32"))
    p.add_argument("--fps", type=int, default=20)
    p.add_argument("--num_clusters", type=int, default=8)
    p.add_argument("--seed", type=int, default=0)
    return p.parse_args(argv)


# ---------------------------------------------------------------------------------------------------- pure host pieces
def scene_frames(directory: str) -> list:
    """The frames of a scene as the script lists them: every entry of the directory, sorted by name."""
    if not os.path.isdir(directory):
        raise _lib.DvtError(f"--frames: {directory} is not a directory")
    names = sorted(os.listdir(directory))
    if not names:
        raise _lib.DvtError(f"--frames: {directory} holds no frames")
    return [os.path.join(directory, n) for n in names]


def scene_name(directory: str) -> str:
    return os.path.basename(os.path.normpath(directory))


def load_frame(path: str, height: int, width: int, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> torch.Tensor:
    """The script's base_transform on the host: RGB, PIL bicubic resize to (width, height), ToTensor, the model's
    normalisation (`model_statistics`).  float32 [3, height, width]."""
    from PIL import Image
    with Image.open(path) as im:
        a = np.array(im.convert("RGB").resize((int(width), int(height)), Image.BICUBIC))  # a writable copy
    t = torch.from_numpy(a).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    mean = torch.as_tensor(mean, dtype=torch.float32).view(3, 1, 1)
    std = torch.as_tensor(std, dtype=torch.float32).view(3, 1, 1)
    return t.sub_(mean).div_(std)


def plan(args) -> dict:
    """Everything that can be refused is refused here, by name, before anything is written: the model, the statistics,
    the geometry (from the extractor's own configuration) and the scenes."""
    if args.model not in _vit.SPECS:
        raise _lib.DvtError(f"--model {args.model}: only {sorted(_vit.SPECS)} are built")
    if not args.vit_checkpoint and not args.allow_random_vit and not os.environ.get("DVT_VIT_CHECKPOINT"):
        raise _lib.DvtError("no ViT weights: pass --vit_checkpoint (a stage-3 *_distilled checkpoint or a timm state dict) or "
                            "--allow_random_vit")
    if args.vit_checkpoint and not os.path.isfile(args.vit_checkpoint):
        raise _lib.DvtError(f"--vit_checkpoint: {args.vit_checkpoint} does not exist")
    if args.fps < 1:
        raise _lib.DvtError(f"--fps {args.fps} must be positive")
    _vit.require_consumer_width(args.model, "visualisation / video (DVT_VIS_MAX_C)")
    spec = _vit.SPECS[args.model]
    if args.height < spec.patch or args.width < spec.patch or args.stride_size < 1:
        raise _lib.DvtError(f"--height {args.height} --width {args.width} --stride_size {args.stride_size}: the frame must hold "
                            f"one {spec.patch}-pixel patch and the stride must be positive")
    cfg = _vit.vit_config(spec.dim, spec.depth, spec.patch, args.stride_size, args.height, args.width, spec.n_reg,
                          pos_has_cls=spec.pos_has_cls)
    stats = VD.load_stats(args.stats, args.stats_prefix)
    VD.check_geometry((cfg.grid_h, cfg.grid_w), cfg.dim, args.num_clusters, stats)
    scenes = [(scene_name(d), scene_frames(d)) for d in args.frames]
    if len({s for s, _ in scenes}) != len(scenes):
        raise _lib.DvtError("--frames: two scenes share a directory name, their outputs would overwrite each other")
    return {"grid_hw": (cfg.grid_h, cfg.grid_w), "channels": cfg.dim, "stats": stats, "scenes": scenes}


def save_animation(path_stem: str, frames: list, fps: int) -> str:
    """`.mp4` through imageio when it imports, otherwise an animated `.gif` through PIL.  The imageio branch is the script's
    own call; imageio is not installed where this project is tested, so only the `.gif` branch has been run."""
    try:
        import imageio
    except ImportError:
        imageio = None
    if imageio is not None:
        path = path_stem + ".mp4"
        imageio.mimsave(path, frames, fps=fps)
        return path
    path = path_stem + ".gif"
    frames[0].save(path, save_all=True, append_images=frames[1:], duration=1000 / fps, loop=0)
    return path


# ---------------------------------------------------------------------------------------------------- the run
def main(args, device=None) -> dict:
    from PIL import Image

    from .models import PretrainedViTWrapper
    todo = plan(args)
    if device is None:
        device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(device)
    vit = PretrainedViTWrapper(args.model, stride=args.stride_size, checkpoint_path=args.vit_checkpoint,
                               img_size=(args.height, args.width), allow_random_init=args.allow_random_vit, dtype=args.dtype)
    eng = VD.VideoDemoEngine(device, todo["grid_hw"], todo["channels"], (args.height, args.width), todo["stats"],
                             args.num_clusters, args.seed, *model_statistics(args.model))
    try:
        import imageio  # noqa: F401
    except ImportError:
        print("dvt_amd.video_demo: imageio is not installed, the animations are written as .gif through PIL", flush=True)

    writes: queue.Queue = queue.Queue(maxsize=2)
    errors = []
    videos: dict = {}

    def writer():
        while True:
            item = writes.get()
            if item is None:
                return
            try:
                host, event, scene, i = item
                event.synchronize()
                arr = host.numpy()
                for k, kind in enumerate(VD.KINDS):
                    img = Image.fromarray(arr[k])
                    img.save(os.path.join(args.output_dir, scene, "images", f"{i:02d}_{kind}.png"))
                    videos[scene][kind].append(img)
            except BaseException as e:  # noqa: BLE001 - re-raised by the run
                errors.append(e)

    th = threading.Thread(target=writer, name="dvt-video-writer", daemon=True)
    th.start()
    start, done, written = time.time(), 0, []
    try:
        for scene, frames in todo["scenes"]:
            os.makedirs(os.path.join(args.output_dir, scene, "images"), exist_ok=True)
            videos[scene] = {k: [] for k in VD.KINDS}
            for i, path in enumerate(frames):
                if errors:
                    break
                img = load_frame(path, args.height, args.width, *model_statistics(args.model)).pin_memory().to(device, non_blocking=True)
                feats = vit.features_nhwc(img[None])
                if i == 0:
                    eng.fit(feats)
                eng.frame(feats, image=img)
                host = torch.empty(eng.full.shape, dtype=torch.uint8, pin_memory=True)
                host.copy_(eng.full, non_blocking=True)
                event = torch.cuda.Event()
                event.record()
                writes.put((host, event, scene, i))
                done += 1
    finally:
        writes.put(None)
        th.join()
    if errors:
        raise errors[0]
    for scene, _ in todo["scenes"]:
        for kind in VD.KINDS:
            written.append(save_animation(os.path.join(args.output_dir, scene, VD.VIDEO_NAMES[kind]), videos[scene][kind],
                                          args.fps))
    print(f"{done} frames of {len(todo['scenes'])} scene(s) in {time.time() - start:.1f}s -> {args.output_dir}", flush=True)
    return {"frames": done, "animations": written}


if __name__ == "__main__":
    main(get_args())
