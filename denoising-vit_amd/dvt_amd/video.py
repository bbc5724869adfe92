"""Host side of the feature-video demo (csrc/dvt_video.hip, C ABI in include/dvt_video.h).

`VideoDemoEngine` restates what the reference's `make_video_demo.py` does with a frame's features: the instance PCA basis,
the k-means centres and the two foreground PCA bases are fitted ONCE, on frame 0 (`fit`, through `dvt_amd.vis.VisEngine`),
and every frame (`frame`) only applies them: one pass over the features gives all thirteen projection columns, the row
norms and the cluster labels; the per-frame column ranges, the softmax-of-norm map, the two foreground masks, the nine
token-resolution uint8 pictures and their Pillow-exact bicubic resize follow on [n, 13] projections and uint8 pictures.
Nothing in `frame` waits for the device.

The pure host pieces (Pillow's resampling tables, the uint8 colour tables, the statistics file, the geometry check) are
plain numpy, so that they can be checked without a GPU.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from . import vis as V

_P, _I, _F = C.c_void_p, C.c_int, C.c_float
_lib.register_signatures({
    "dvt_video_apply": (_I, [_P, _I, _I, _P, _I, _P, _I, _P, _P, _P, _P]),
    "dvt_video_col_range": (_I, [_P, _I, _I, _P, _I, _F, _F, _P, _P]),
    "dvt_video_softmax_norm_map": (_I, [_P, _I, _F, _P, _P]),
    "dvt_video_threshold_mask": (_I, [_P, _I, _I, _I, _F, _F, _F, _P, _P]),
    "dvt_video_picture_rgb": (_I, [_P, _I, _I, _I, _P, _P, _P, _P]),
    "dvt_video_picture_scalar": (_I, [_P, _I, _I, _I, _I, _F, _F, _P, _I, _P, _P, _P]),
    "dvt_video_picture_labels": (_I, [_P, _I, _P, _I, _P, _P]),
    "dvt_video_denorm_u8": (_I, [_P, _I, _I, _P, _P, _P, _P]),
    "dvt_video_resize_bicubic_u8": (_I, [_P, _I, _I, _I, _P, _I, _I, _P, _P, _I, _P, _P, _I, _P, _P]),
})

MAX_M, MAX_TAPS, MAX_IMAGES = 32, 64, 64
# the ten pictures of a frame, in the script's order, and the names of its animations
KINDS = ("input", "pca_instance", "pca_dataset", "kmeans", "first_pca", "second_pca", "third_pca", "fg_pca",
         "fg_pca_standard", "norm")
VIDEO_NAMES = {"input": "image", "pca_instance": "instance_pca", "pca_dataset": "dataset_pca", "kmeans": "kmeans",
               "first_pca": "first_pca", "second_pca": "second_pca", "third_pca": "third_pca", "fg_pca": "fg_pca",
               "norm": "norm", "fg_pca_standard": "fg_pca_standard"}
MAP_KINDS = KINDS[1:]
# columns of the projection matrix M [C, 13]
COL_INSTANCE, COL_DATASET, COL_STANDARD, COL_FG, COL_FG_STANDARD, N_COLS = 0, 3, 6, 7, 10, 13
FG_THRESHOLD = 0.1      # 1 - pca_full[..., 1] > 0.1
NORM_TEMPERATURE = 5.0  # softmax(|x| / 5)
STATS_KEYS = ("reduct_mat_full", "standard_mapping")


# ================================================================================================ pure host pieces
def _bicubic(x: float) -> float:
    """Pillow's bicubic_filter (Keys, a = -0.5), operation by operation."""
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def bicubic_tables(in_size: int, out_size: int):
    """Pillow's `precompute_coeffs` + `normalize_coeffs_8bpc` for the bicubic filter over the whole axis, in float64:
    (bounds int32 [out, 2] = (first source index, taps), coefficients int32 [out, ksize], fixed point with 22 bits)."""
    in_size, out_size = int(in_size), int(out_size)
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        bounds[xx] = (xmin, xmax)
        for x, w in enumerate(k):
            coef[xx, x] = int(-0.5 + w * (1 << 22)) if w < 0 else int(0.5 + w * (1 << 22))
    return bounds, coef


def color_table_u8(name: str) -> np.ndarray:
    """uint8 [256, 3]: `(plt.get_cmap(name)(v)[:3] * 255).astype(np.uint8)` for every entry of the 256-entry table (the
    colours are float64 there, so the conversion is done here, once, in float64)."""
    try:
        import matplotlib
    except ImportError as exc:  # pragma: no cover - matplotlib is a dependency of the reference too
        raise _lib.DvtError("the video demo reads its colour tables (inferno, rainbow) from matplotlib, which is not "
                            "installed") from exc
    lut = matplotlib.colormaps[name](np.arange(256))[:, :3]
    return np.ascontiguousarray((lut * 255).astype(np.uint8))


def label_table_u8(name: str, num_clusters: int) -> np.ndarray:
    """uint8 [K, 3]: the script's `cmap(labels / K)` per label (labels are float32 there)."""
    v = np.arange(int(num_clusters), dtype=np.float32) / int(num_clusters)
    idx = np.minimum((v * np.float32(256)).astype(np.int64), 255)
    return np.ascontiguousarray(color_table_u8(name)[idx])


def denormalizer(mean, std):
    """(mean, std) float32 [3] of the script's inverse `transforms.Normalize`."""
    return (np.asarray([-m / s for m, s in zip(mean, std)], np.float32),
            np.asarray([1 / s for s in std], np.float32))


def load_stats(path: str, prefix: str = "denoised") -> dict:
    """The reference's `demo/assets/stats.pth` or an `.npz` with the same arrays -> {"reduct_mat_full": float32 [C, 3],
    "standard_mapping": float32 [C, 1]} of `prefix` (denoised | dinov2)."""
    if prefix not in ("denoised", "dinov2"):
        raise _lib.DvtError(f"--stats_prefix must be denoised or dinov2, not {prefix!r}")
    if not os.path.isfile(path):
        raise _lib.DvtError(f"--stats: {path} does not exist")
    if path.endswith(".npz"):
        with np.load(path) as z:
            raw = {k: z[k] for k in z.files}
    else:
        raw = torch.load(path, map_location="cpu", weights_only=True)
    out = {}
    for key, cols in zip(STATS_KEYS, (3, 1)):
        name = f"{prefix}_{key}"
        if name not in raw:
            raise _lib.DvtError(f"--stats: {path} has no array {name!r} (found {sorted(raw)})")
        a = raw[name]
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        if a.ndim != 2 or a.shape[1] != cols:
            raise _lib.DvtError(f"--stats: {name} has shape {tuple(a.shape)}, expected [C, {cols}]")
        out[key] = np.ascontiguousarray(a, dtype=np.float32)
    if out["reduct_mat_full"].shape[0] != out["standard_mapping"].shape[0]:
        raise _lib.DvtError("--stats: the two arrays differ in their channel count")
    return out


def check_geometry(grid_hw, channels: int, num_clusters: int = 8, stats: dict | None = None) -> None:
    """Refuse, by name, what the library cannot take -- before anything is written."""
    gh, gw = int(grid_hw[0]), int(grid_hw[1])
    if gh < 1 or gw < 1 or gh * gw > V.MAX_ROWS:
        raise _lib.DvtError(f"a token grid of {gh} x {gw} = {gh * gw} rows exceeds DVT_VIS_MAX_ROWS = {V.MAX_ROWS}")
    if channels % 64 or not 64 <= channels <= V.MAX_C:
        raise _lib.DvtError(f"{channels} channels: the visualisation kernels need a multiple of 64 in [64, DVT_VIS_MAX_C = "
                            f"{V.MAX_C}]")
    if not 1 <= int(num_clusters) <= V.MAX_K:
        raise _lib.DvtError(f"--num_clusters {num_clusters} is outside [1, DVT_VIS_MAX_K = {V.MAX_K}]")
    if gh * gw < int(num_clusters):
        raise _lib.DvtError(f"{num_clusters} clusters need at least as many tokens, the grid has {gh * gw}")
    if stats is not None and stats["reduct_mat_full"].shape[0] != channels:
        raise _lib.DvtError(f"--stats was made for {stats['reduct_mat_full'].shape[0]} channels, the model has {channels}")


# ================================================================================================ the engine
class VideoDemoEngine:
    """The per-frame pictures of the video demo on one device.  Features are fp32 HIP tensors [grid_h, grid_w, C] (or
    [1, grid_h, grid_w, C] / [n, C]); CPU tensors raise DvtError, there is no CPU fallback.

    What `frame` returns lives in buffers this engine owns: it is valid until the next `frame` call."""

    def __init__(self, device, grid_hw, channels: int, out_hw, stats: dict, num_clusters: int = 8, seed: int = 0,
                 norm_mean=(0.485, 0.456, 0.406), norm_std=(0.229, 0.224, 0.225)):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DvtError("the video demo needs a HIP device; there is no CPU fallback")
        self.gh, self.gw = int(grid_hw[0]), int(grid_hw[1])
        self.H, self.W = int(out_hw[0]), int(out_hw[1])
        self.C, self.K, self.seed = int(channels), int(num_clusters), int(seed)
        check_geometry((self.gh, self.gw), self.C, self.K, stats)
        self.n = self.gh * self.gw
        self.vis = V.VisEngine(self.device, max_rows=self.n, max_channels=self.C, max_clusters=self.K)
        up = self.vis.upload
        self.dataset = up(stats["reduct_mat_full"])        # [C, 3]
        self.standard = up(stats["standard_mapping"])      # [C, 1]
        self.inferno = up(color_table_u8("inferno"), torch.uint8)
        self.label_colors = up(label_table_u8("rainbow", self.K), torch.uint8)
        dm, ds = denormalizer(norm_mean, norm_std)
        self.denorm_mean, self.denorm_std = up(dm), up(ds)
        xb, xc = bicubic_tables(self.gw, self.W)
        yb, yc = bicubic_tables(self.gh, self.H)
        if xc.shape[1] > MAX_TAPS or yc.shape[1] > MAX_TAPS:
            raise _lib.DvtError(f"resizing {self.gh} x {self.gw} to {self.H} x {self.W} needs more than {MAX_TAPS} filter taps")
        self.xb, self.xc, self.yb, self.yc = (up(a, torch.int32) for a in (xb, xc, yb, yc))
        new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=self.device)  # noqa: E731
        n, nm = self.n, len(MAP_KINDS)
        self.P, self.norms, self.labels = new((n, N_COLS)), new(n), new(n, torch.int32)
        self.range, self.range_second, self.norm_map = new((2, N_COLS)), new(2), new(n)
        self.mask_fg, self.mask_standard = new(n, torch.uint8), new(n, torch.uint8)
        self.P0 = new((n, 4))
        self.token = new((nm, self.gh, self.gw, 3), torch.uint8)
        self.tmp = new((nm, self.gh, self.W, 3), torch.uint8)
        self.full = new((len(KINDS), self.H, self.W, 3), torch.uint8)
        self.M = self.centers = None
        self.launches = 0
        self._printed = False

    # ---- helpers ----------------------------------------------------------------------------------
    def _rows(self, feats: torch.Tensor) -> torch.Tensor:
        _lib.require_cuda(feats)
        if feats.shape[-1] != self.C or feats.numel() != self.n * self.C:
            raise _lib.DvtError(f"features {tuple(feats.shape)}: this engine was made for a {self.gh} x {self.gw} x {self.C} map")
        return feats.detach().to(torch.float32).reshape(self.n, self.C).contiguous()

    def _call(self, name: str, *args, launches: int = 1) -> None:
        _lib.check(getattr(_lib.lib(), name)(*args, _lib.stream()), name)
        self.launches += launches

    def apply(self, x, M, centers, P, norms, labels) -> None:
        self._call("dvt_video_apply", x.data_ptr(), x.shape[0], x.shape[1], M.data_ptr(), M.shape[1], _lib.ptr(centers),
                   0 if centers is None else centers.shape[0], P.data_ptr(), _lib.ptr(norms), _lib.ptr(labels))

    def threshold(self, P, col: int, s: float, o: float, t: float, mask) -> None:
        self._call("dvt_video_threshold_mask", P.data_ptr(), P.shape[0], P.shape[1], col, s, o, t, mask.data_ptr())

    def resize(self, src: torch.Tensor, dst: torch.Tensor, tmp: torch.Tensor) -> None:
        """src uint8 [k, gh, gw, 3] -> dst uint8 [k, H, W, 3] (contiguous), Pillow's bicubic."""
        self._call("dvt_video_resize_bicubic_u8", src.data_ptr(), src.shape[0], self.gh, self.gw, dst.data_ptr(), self.H, self.W,
                   self.xb.data_ptr(), self.xc.data_ptr(), self.xc.shape[1], self.yb.data_ptr(), self.yc.data_ptr(),
                   self.yc.shape[1], tmp.data_ptr(), launches=2)

    # ---- frame 0 ----------------------------------------------------------------------------------
    def fit(self, feats0: torch.Tensor) -> dict:
        """Fit on frame 0: the instance basis (robust PCA, m = 2), the cosine k-means centres (start rows from `seed`) and the
        two foreground bases (PCA over the rows of either foreground mask).  Returns them (device tensors).
        Precondition: each foreground mask selects at least two rows of frame 0.  The masks live on the device and `fit` does not
        wait for it, so this is not checked: for fewer rows `dvt_vis_pca_basis` writes a zero basis (include/dvt_vis.h), the
        three projections of that kind are 0 in every frame, their range is empty, and the `fg_pca` / `fg_pca_standard` picture
        is black for the whole scene (0 / 0 is written as 0), where the reference's `torch.pca_lowrank` would raise."""
        x = self._rows(feats0)
        inst, _, _ = self.vis.robust_pca(x, m=2.0)
        rows = V.kmeans_start_rows(self.n, self.K, V.KMEANS_NUM_INIT, np.random.RandomState(self.seed))
        self.centers = self.vis.kmeans(x, self.K, init_rows=rows)["centers"]
        m0 = torch.cat([self.dataset, self.standard], 1).contiguous()
        self.apply(x, m0, None, self.P0, None, None)
        self.threshold(self.P0, 1, -1.0, 1.0, FG_THRESHOLD, self.mask_fg)
        self.threshold(self.P0, 3, 1.0, 0.0, 0.0, self.mask_standard)
        fg, _ = self.vis.pca_basis(x, self.mask_fg)
        fg_standard, _ = self.vis.pca_basis(x, self.mask_standard)
        self.M = torch.cat([inst, self.dataset, self.standard, fg, fg_standard], 1).contiguous()
        return {"instance": inst, "centers": self.centers, "fg": fg, "fg_standard": fg_standard, "M": self.M}

    # ---- every frame ------------------------------------------------------------------------------
    def frame(self, feats: torch.Tensor, image: torch.Tensor | None = None, details: bool = False):
        """dict kind -> uint8 [H, W, 3] device tensor for the nine feature pictures, plus `input` when `image` (the normalised
        frame, fp32 [3, H, W] or [1, 3, H, W] on the device) is given.  details=True: (pictures, dict of P, norms, labels,
        masks, ranges, norm_map and the token-resolution pictures)."""
        if self.M is None:
            raise _lib.DvtError("VideoDemoEngine.frame before fit: the bases and centres come from frame 0")
        x = self._rows(feats)
        first = self.launches
        n, m = self.n, N_COLS
        P, tok = self.P, self.token.view(len(MAP_KINDS), n, 3)
        self.apply(x, self.M, self.centers, P, self.norms, self.labels)
        self._call("dvt_video_col_range", P.data_ptr(), n, m, self.range.data_ptr(), COL_DATASET + 1, -1.0, 1.0,
                   self.range_second.data_ptr())
        self._call("dvt_video_softmax_norm_map", self.norms.data_ptr(), n, NORM_TEMPERATURE, self.norm_map.data_ptr())
        self.threshold(P, COL_DATASET + 1, -1.0, 1.0, FG_THRESHOLD, self.mask_fg)
        self.threshold(P, COL_STANDARD, 1.0, 0.0, 0.0, self.mask_standard)
        at = {k: tok[i] for i, k in enumerate(MAP_KINDS)}
        for kind, col, mask in (("pca_instance", COL_INSTANCE, None), ("pca_dataset", COL_DATASET, None),
                                ("fg_pca", COL_FG, self.mask_fg), ("fg_pca_standard", COL_FG_STANDARD, self.mask_standard)):
            self._call("dvt_video_picture_rgb", P.data_ptr(), n, m, col, self.range.data_ptr(), _lib.ptr(mask),
                       at[kind].data_ptr())
        self._call("dvt_video_picture_labels", self.labels.data_ptr(), n, self.label_colors.data_ptr(), self.K,
                   at["kmeans"].data_ptr())
        col_range = lambda c: (self.range.data_ptr() + 4 * c, m)  # noqa: E731  (lo, hi of column c: m floats apart)
        for kind, col, aff, (r, rs) in (("first_pca", COL_DATASET, 0, col_range(COL_DATASET)),
                                        ("second_pca", COL_DATASET + 1, 1, (self.range_second.data_ptr(), 1)),
                                        ("third_pca", COL_DATASET + 2, 0, col_range(COL_DATASET + 2))):
            self._call("dvt_video_picture_scalar", P.data_ptr(), n, m, col, aff, -1.0, 1.0, r, rs, self.inferno.data_ptr(),
                       at[kind].data_ptr())
        self._call("dvt_video_picture_scalar", self.norm_map.data_ptr(), n, 1, 0, 0, 1.0, 0.0, None, 1, self.inferno.data_ptr(),
                   at["norm"].data_ptr())
        self.resize(self.token, self.full[1:], self.tmp)
        out = {k: self.full[1 + i] for i, k in enumerate(MAP_KINDS)}
        if image is not None:
            _lib.require_cuda(image)
            img = image.detach().to(torch.float32).reshape(3, self.H, self.W).contiguous()
            self._call("dvt_video_denorm_u8", img.data_ptr(), self.H, self.W, self.denorm_mean.data_ptr(),
                       self.denorm_std.data_ptr(), self.full[0].data_ptr())
            out = {"input": self.full[0], **out}
        if not self._printed:
            self._printed = True
            print(f"dvt_amd.video: {self.launches - first} kernel launches per frame", flush=True)
        if not details:
            return out
        return out, {"P": P, "norms": self.norms, "labels": self.labels, "mask_fg": self.mask_fg,
                     "mask_standard": self.mask_standard, "range": self.range, "range_second": self.range_second,
                     "norm_map": self.norm_map, "token": {k: self.token[i] for i, k in enumerate(MAP_KINDS)}}
