"""Records what the reference's make_video_demo.py computes per frame, for tests/test_video_cpu.py.  Run by hand next to the
reference:

    python tests/golden/make_video_golden.py /path/to/reference

The script is flat and loads a model at import, so it cannot be imported.  This maker reads its text at run time, takes the
per-frame statements (from `# 2. instance pca` inside the frame loop to the last `norm_video.append`), and executes them in
a namespace that supplies `feat`, the fitted matrices, a stand-in `kmeans.predict`, the colour maps, the grid size (the
literal `120, 211` and the literal channel count rewritten in memory) and a stand-in `Image` that records every array handed
to `Image.fromarray`: the nine token-resolution uint8 pictures.  `i = 1`, so the script's `if i == 0` fits are skipped and
the given foreground bases are used.  The features are float64 tensors: the statements do not name a dtype, and
tests/video_reference.py restates them in float64.

Writes (data only, never the script's text):
  video_reference.npz          inputs and the nine pictures of two small seeded maps
  video_reference_flags.json   the script's constants
  video_stats.npz              the four arrays of demo/assets/stats.pth
  davis-mallard-water/         frames 00000.jpg and 00040.jpg of the demo scene
"""
import json
import os
import re
import shutil
import sys
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import video_reference as R  # noqa: E402

KINDS = R.MAP_KINDS
CASES = {"a": ((9, 13, 64), 8, 3), "b": ((12, 10, 128), 5, 4)}  # shape, clusters, seed


class _Picture:
    def resize(self, *a, **k):
        return self

    def save(self, *a, **k):
        pass


class _Image:
    BICUBIC = 3

    def __init__(self):
        self.arrays = []

    def fromarray(self, a):
        self.arrays.append(np.array(a, copy=True))
        return _Picture()


class _KMeans:
    def __init__(self, centers):
        self.centers = centers

    def predict(self, x):
        labels, _ = R.kmeans_predict(x[0].numpy(), self.centers)
        return torch.from_numpy(labels)[None]


def frame_statements(text: str) -> str:
    lines = text.splitlines()
    starts = [k for k, l in enumerate(lines) if l.strip() == "# 2. instance pca"]
    first = starts[-1]  # the second occurrence: the per-frame one (the first sits under `if i == 0`)
    last = max(k for k, l in enumerate(lines) if "norm_video.append" in l)
    return textwrap.dedent("\n".join(lines[first:last + 1]))


def constants(text: str) -> dict:
    grab = lambda pat: re.search(pat, text, re.M).group(1)  # noqa: E731
    h, w = re.search(r"^h, w = (\d+), (\d+)", text, re.M).groups()
    return {"model": grab(r'^vit_type = "([^"]+)"'), "stride_size": int(grab(r"^stride = (\d+)")), "height": int(h),
            "width": int(w), "patch_size": int(grab(r"^patch_size = (\d+)")), "fps": int(grab(r"fps=(\d+)")),
            "num_clusters": int(grab(r"n_clusters=(\d+)")), "output_dir": grab(r'^output_path = "([^"]+)"'),
            "norm_temperature": int(grab(r"norm\.reshape\(1, -1\) / (\d+)")),
            "fg_threshold": float(grab(r"pca_full\[\.\.\., 1\] > ([0-9.]+)")),
            "token_grid": [int(v) for v in re.search(r"reshape\((\d+), (\d+), 3\)", text).groups()]}


def main(ref_root: str) -> None:
    import matplotlib.pyplot as plt
    import torch.nn.functional as F
    text = open(os.path.join(ref_root, "make_video_demo.py")).read()
    flags = constants(text)
    body = frame_statements(text)
    out = {}
    for name, ((gh, gw, c), k, seed) in CASES.items():
        rng = np.random.RandomState(seed)
        x = R.seeded_feature_map((gh, gw, c), seed)
        mats = {n: rng.standard_normal((c, 3)).astype(np.float32) / np.sqrt(c) for n in ("instance", "dataset", "fg", "fg_standard")}
        mats["standard"] = rng.standard_normal((c, 1)).astype(np.float32) / np.sqrt(c)
        centers = x.reshape(-1, c)[rng.choice(gh * gw, k, replace=False)].copy()
        code = body.replace("120, 211", f"{gh}, {gw}").replace("-1, 768", f"-1, {c}").replace("/ 8)", f"/ {k})")
        image = _Image()
        t64 = lambda a: torch.from_numpy(a.astype(np.float64))  # noqa: E731
        ns = {"torch": torch, "np": np, "F": F, "os": os, "Image": image, "feat": t64(x)[None], "i": 1, "h": 1, "w": 1,
              "scene": "scene", "output_path": "unused", "instance_reduct_mat": t64(mats["instance"]),
              "dataset_reduct_mat": t64(mats["dataset"]), "dataset_reduct_mat_standard": t64(mats["standard"]),
              "fg_pca_reduct": t64(mats["fg"]), "fg_pca_reduct2": t64(mats["fg_standard"]), "kmeans": _KMeans(centers),
              "cmap": plt.get_cmap("rainbow"), "inferno_cmap": plt.get_cmap("inferno")}
        for v in ("instance_pca", "dataset_pca", "kmeans", "first_pca", "second_pca", "third_pca", "fg_pca", "norm",
                  "fg_pca_standard"):
            ns[v + "_video"] = []
        exec(compile(code, "<frame statements>", "exec"), ns)  # noqa: S102
        assert len(image.arrays) == len(KINDS), len(image.arrays)
        out[f"{name}.x"], out[f"{name}.centers"] = x, centers
        out[f"{name}.clusters"] = np.int32(k)
        for n, m in mats.items():
            out[f"{name}.{n}"] = m
        for kind, a in zip(KINDS, image.arrays):
            assert a.dtype == np.uint8 and a.shape == (gh, gw, 3), (kind, a.dtype, a.shape)
            out[f"{name}.{kind}"] = a
    np.savez_compressed(os.path.join(HERE, "video_reference.npz"), **out)
    json.dump(flags, open(os.path.join(HERE, "video_reference_flags.json"), "w"), indent=1)
    stats = torch.load(os.path.join(ref_root, "demo", "assets", "stats.pth"), map_location="cpu", weights_only=True)
    np.savez_compressed(os.path.join(HERE, "video_stats.npz"), **{k: v.numpy() for k, v in stats.items()})
    scene = os.path.join(HERE, "davis-mallard-water")
    os.makedirs(scene, exist_ok=True)
    for f in ("00000.jpg", "00040.jpg"):
        shutil.copyfile(os.path.join(ref_root, "demo", "davis-mallard-water", f), os.path.join(scene, f))
    print(flags)


if __name__ == "__main__":
    main(sys.argv[1])
