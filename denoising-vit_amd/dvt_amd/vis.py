"""Host side of the feature-map visualisation (csrc/dvt_vis.hip, C ABI in include/dvt_vis.h).

`VisEngine` owns the workspace, the colour tables and the canvas on one device and exposes the pieces of the reference's
`dvt/utils/visualization/visualization_tools.py` as device operations: the robust PCA colours, the norm and similarity
maps, cosine k-means, and the rendering of each into a rectangle of one canvas, which leaves the device in one copy.
Every call enqueues on the current stream and none waits for the device: host arrays (k-means start rows, label bitmaps)
go up through pinned memory with non-blocking copies (`VisEngine.upload`), colour tables and label bitmaps once.

The pure host pieces (colour tables from matplotlib, k-means start rows, the tile geometry) are plain Python, so that they
can be checked without a GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

_P, _I, _I64, _F = C.c_void_p, C.c_int, C.c_int64, C.c_float
_lib.register_signatures({
    "dvt_vis_workspace_bytes": (_I64, [_I, _I, _I, _I]),
    "dvt_vis_pca_basis": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _I64, _P]),
    "dvt_vis_project": (_I, [_P, _P, _P, _P, _I, _I, _P, _P]),
    "dvt_vis_robust_range": (_I, [_P, _P, _I, _F, _P, _P, _P, _P, _I64, _P]),
    "dvt_vis_fg_mask": (_I, [_P, _I, _F, _P, _P]),
    "dvt_vis_norm_map": (_I, [_P, _I, _I, _P, _P, _I64, _P]),
    "dvt_vis_similarity_map": (_I, [_P, _I, _I, _I, _P, _P, _I64, _P]),
    "dvt_vis_kmeans": (_I, [_P, _I, _I, _I, _P, _P, _I, _I, _F, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "dvt_vis_render_scalar": (_I, [_P, _I, _I, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "dvt_vis_render_rgb": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "dvt_vis_render_labels": (_I, [_P, _I, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "dvt_vis_fill": (_I, [_P, _I, _I, _I, _I, _I, _I, _F, _F, _F, _P]),
    "dvt_vis_canvas_to_u8": (_I, [_P, _I, _I, _P, _P]),
})

MAX_C, MAX_ROWS, MAX_K, MAX_INIT, MAX_ITER = 1024, 65536, 16, 16, 1000
PCA_ITERS = 48          # orthogonal-iteration steps of the PCA basis
KMEANS_TOL = 1e-4       # torch_kmeans' documented defaults
KMEANS_MAX_ITER = 100
KMEANS_NUM_INIT = 8
INTERP = {"nearest": 0, "bilinear": 1}


# ================================================================================================ pure host pieces
def color_table(name: str, entries: int = 256) -> np.ndarray:
    """A matplotlib colour map as a float32 [entries, 3] table (`plt.get_cmap(name, entries)` evaluated at its own entries).
    With 256 entries, `table[min(int(v * 256), 255)]` is what `plt.get_cmap(name)(v)` returns for v in [0, 1]."""
    try:
        import matplotlib
    except ImportError as exc:  # pragma: no cover - matplotlib is a dependency of the reference too
        raise _lib.DvtError("the visualisation reads its colour tables (inferno, turbo, rainbow) from matplotlib, which is "
                            "not installed") from exc
    cmap = matplotlib.colormaps[name].resampled(int(entries))
    return np.ascontiguousarray(cmap(np.arange(int(entries)))[:, :3], dtype=np.float32)


def kmeans_start_rows(n: int, num_clusters: int, num_init: int, rng: np.random.RandomState) -> np.ndarray:
    """Start rows of every restart: `num_clusters` distinct rows each, drawn from the CALLER's generator."""
    return np.stack([rng.choice(n, size=num_clusters, replace=False) for _ in range(num_init)]).astype(np.int32)


# ================================================================================================ the engine
class VisEngine:
    """Visualisation kernels on one device.  Feature maps are fp32 CUDA(HIP) tensors [..., C] (any leading shape, made
    contiguous); CPU tensors raise DvtError, there is no CPU fallback."""

    def __init__(self, device, max_rows: int = 8 * 37 * 37, max_channels: int = MAX_C, max_clusters: int = MAX_K,
                 max_init: int = KMEANS_NUM_INIT):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DvtError("the visualisation needs a HIP device; there is no CPU fallback")
        self.max_rows, self.max_channels = int(max_rows), int(max_channels)
        self.max_clusters, self.max_init = int(max_clusters), int(max_init)
        nbytes = int(_lib.lib().dvt_vis_workspace_bytes(self.max_rows, self.max_channels, self.max_clusters, self.max_init))
        if nbytes < 0:
            raise _lib.DvtError(f"dvt_vis_workspace_bytes({max_rows}, {max_channels}, {max_clusters}, {max_init}): bad arguments")
        self.work = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.canvas = None
        self._tables = {}
        self._label_bitmaps = {}  # tile labels on the device, by (text, font): utils.visualization

    # ---- helpers ----------------------------------------------------------------------------------
    def _rows(self, feats: torch.Tensor) -> torch.Tensor:
        _lib.require_cuda(feats)
        x = feats.detach().to(torch.float32).reshape(-1, feats.shape[-1]).contiguous()
        n, c = x.shape
        if n > self.max_rows or c > self.max_channels:
            raise _lib.DvtError(f"a map of {n} rows x {c} channels exceeds this engine's workspace ({self.max_rows} x "
                                f"{self.max_channels})")
        return x

    def _new(self, shape, dtype=torch.float32) -> torch.Tensor:
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _wk(self):
        return self.work.data_ptr(), self.work.numel()

    def upload(self, array, dtype=torch.float32) -> torch.Tensor:
        """A host array on the device through pinned memory and a non-blocking copy: the host does not wait for the stream
        (a copy from pageable memory would).  Device tensors pass through."""
        if torch.is_tensor(array) and array.is_cuda:
            return array.to(self.device, dtype)
        host = torch.as_tensor(array).to(dtype).contiguous()
        return host.pin_memory().to(self.device, non_blocking=True)

    def table(self, name: str, entries: int = 256) -> torch.Tensor:
        """The device copy of a colour table, uploaded once."""
        key = (name, int(entries))
        if key not in self._tables:
            self._tables[key] = self.upload(color_table(name, entries))
        return self._tables[key]

    # ---- PCA --------------------------------------------------------------------------------------
    def pca_basis(self, feats: torch.Tensor, mask: torch.Tensor | None = None, iters: int = PCA_ITERS):
        """(basis [C, 3], eigenvalues [3]) of the rows selected by mask (uint8 / bool [n], None: all)."""
        x = self._rows(feats)
        m = None
        if mask is not None:
            _lib.require_cuda(mask)
            m = mask.reshape(-1).to(torch.uint8).contiguous()
            if m.numel() != x.shape[0]:
                raise _lib.DvtError("mask and rows differ in length")
        basis, evals = self._new((x.shape[1], 3)), self._new(3)
        w, wb = self._wk()
        _lib.check(_lib.lib().dvt_vis_pca_basis(x.data_ptr(), _lib.ptr(m), x.shape[0], x.shape[1], int(iters), basis.data_ptr(),
                                                evals.data_ptr(), w, wb, _lib.stream()), "dvt_vis_pca_basis")
        return basis, evals

    def project(self, feats: torch.Tensor, basis: torch.Tensor, rgb_min: torch.Tensor | None = None,
                rgb_max: torch.Tensor | None = None) -> torch.Tensor:
        """[n, 3] = rows @ basis, range-normalised and clamped to [0, 1] when a range is given."""
        x = self._rows(feats)
        _lib.require_cuda(basis, rgb_min, rgb_max)
        basis = basis.to(torch.float32).contiguous()
        if tuple(basis.shape) != (x.shape[1], 3):
            raise _lib.DvtError(f"basis {tuple(basis.shape)}, expected {(x.shape[1], 3)}")
        lo = None if rgb_min is None else rgb_min.to(self.device, torch.float32).contiguous()
        hi = None if rgb_max is None else rgb_max.to(self.device, torch.float32).contiguous()
        out = self._new((x.shape[0], 3))
        _lib.check(_lib.lib().dvt_vis_project(x.data_ptr(), basis.data_ptr(), _lib.ptr(lo), _lib.ptr(hi), x.shape[0], x.shape[1],
                                              out.data_ptr(), _lib.stream()), "dvt_vis_project")
        return out

    def robust_range(self, colors: torch.Tensor, mask: torch.Tensor | None = None, m: float = 2.0, details: bool = False):
        """(rgb_min [3], rgb_max [3]) of projected rows [n, 3]; details=True adds the dict of medians / deviations (fp64 [3]
        each) and the int32 [13] row record of include/dvt_vis.h."""
        _lib.require_cuda(colors, mask)
        colors = colors.to(torch.float32).reshape(-1, 3).contiguous()
        mk = None if mask is None else mask.reshape(-1).to(torch.uint8).contiguous()
        rng = self._new(6)
        stats = self._new(6, torch.float64)
        rows = self._new(13, torch.int32)
        w, wb = self._wk()
        _lib.check(_lib.lib().dvt_vis_robust_range(colors.data_ptr(), _lib.ptr(mk), colors.shape[0], float(m), rng.data_ptr(),
                                                   stats.data_ptr(), rows.data_ptr(), w, wb, _lib.stream()),
                   "dvt_vis_robust_range")
        if details:
            return rng[:3], rng[3:], {"median": stats[:3], "deviation": stats[3:], "rows": rows}
        return rng[:3], rng[3:]

    def fg_mask(self, colors: torch.Tensor, thresh: float = 0.2) -> torch.Tensor:
        _lib.require_cuda(colors)
        colors = colors.to(torch.float32).reshape(-1, 3).contiguous()
        out = self._new(colors.shape[0], torch.uint8)
        _lib.check(_lib.lib().dvt_vis_fg_mask(colors.data_ptr(), colors.shape[0], float(thresh), out.data_ptr(), _lib.stream()),
                   "dvt_vis_fg_mask")
        return out

    def robust_pca(self, feats: torch.Tensor, m: float = 2.0, remove_first_component: bool = False, iters: int = PCA_ITERS):
        """get_robust_pca: (basis [C, 3], rgb_min [3], rgb_max [3]), all on the device."""
        basis, _ = self.pca_basis(feats, None, iters)
        mask = None
        if remove_first_component:
            mask = self.fg_mask(self.project(feats, basis), 0.2)
            basis, _ = self.pca_basis(feats, mask, iters)
        lo, hi = self.robust_range(self.project(feats, basis), mask, m)
        return basis, lo, hi

    def pca_map(self, feat_map: torch.Tensor, pca_stats=None):
        """Colours [h, w, 3] in [0, 1] of a map [h, w, C] (or [1, h, w, C]) and the stats (basis, min, max) that gave them."""
        if pca_stats is None:
            pca_stats = self.robust_pca(feat_map)
        basis, lo, hi = pca_stats
        lead = tuple(feat_map.shape[:-1])
        return self.project(feat_map, basis, lo, hi).reshape(*lead, 3), (basis, lo, hi)

    # ---- scalar maps ------------------------------------------------------------------------------
    def scale_map(self, feat_map: torch.Tensor) -> torch.Tensor:
        """Min-max normalised L2 norms, shape of the map without its channel axis."""
        x = self._rows(feat_map)
        out = self._new(x.shape[0])
        w, wb = self._wk()
        _lib.check(_lib.lib().dvt_vis_norm_map(x.data_ptr(), x.shape[0], x.shape[1], out.data_ptr(), w, wb, _lib.stream()),
                   "dvt_vis_norm_map")
        return out.reshape(tuple(feat_map.shape[:-1]))

    def similarity_map(self, feat_map: torch.Tensor) -> torch.Tensor:
        """[h, w]: min-max normalised cosine with the centre row, the centre itself -1.  feat_map [h, w, C] or [1, h, w, C]."""
        if feat_map.dim() == 4 and feat_map.shape[0] == 1:
            feat_map = feat_map[0]
        if feat_map.dim() != 3:
            raise _lib.DvtError("similarity_map needs one map [h, w, C]")
        h, wd = int(feat_map.shape[0]), int(feat_map.shape[1])
        x = self._rows(feat_map)
        out = self._new((h, wd))
        w, wb = self._wk()
        _lib.check(_lib.lib().dvt_vis_similarity_map(x.data_ptr(), h, wd, x.shape[1], out.data_ptr(), w, wb, _lib.stream()),
                   "dvt_vis_similarity_map")
        return out

    # ---- k-means ----------------------------------------------------------------------------------
    def kmeans(self, feats: torch.Tensor, num_clusters: int, init_rows=None, init_centers=None, max_iter: int = KMEANS_MAX_ITER,
               tol: float = KMEANS_TOL) -> dict:
        """Cosine k-means from the caller's start rows (int [num_init, K]) or start centres ([num_init, K, C]).  Returns device
        tensors: labels int32 [n], centers [K, C], inertia fp64 [num_init], iterations int32 [num_init], best int32 [1]."""
        x = self._rows(feats)
        n, c = x.shape
        K = int(num_clusters)
        rows_t = cen_t = None
        if init_centers is not None:
            cen_t = self.upload(init_centers).reshape(-1, K, c).contiguous()
            num_init = cen_t.shape[0]
        elif init_rows is not None:
            rows_t = self.upload(init_rows, torch.int32).reshape(-1, K).contiguous()
            num_init = rows_t.shape[0]
        else:
            raise _lib.DvtError("kmeans needs init_rows or init_centers: the kernels draw no random numbers")
        if K > self.max_clusters or num_init > self.max_init:
            raise _lib.DvtError(f"{K} clusters x {num_init} restarts exceed this engine's workspace ({self.max_clusters} x "
                                f"{self.max_init})")
        out = {"labels": self._new(n, torch.int32), "centers": self._new((K, c)),
               "inertia": self._new(num_init, torch.float64), "iterations": self._new(num_init, torch.int32),
               "best": self._new(1, torch.int32)}
        w, wb = self._wk()
        _lib.check(_lib.lib().dvt_vis_kmeans(x.data_ptr(), n, c, K, _lib.ptr(rows_t), _lib.ptr(cen_t), int(num_init), int(max_iter),
                                             float(tol), out["labels"].data_ptr(), out["centers"].data_ptr(),
                                             out["inertia"].data_ptr(), out["iterations"].data_ptr(), out["best"].data_ptr(),
                                             w, wb, _lib.stream()), "dvt_vis_kmeans")
        return out

    def cluster_map(self, feat_map: torch.Tensor, num_clusters: int = 10, rng: np.random.RandomState | None = None,
                    seed: int = 0, num_init: int = KMEANS_NUM_INIT) -> torch.Tensor:
        """Labels int32 with the map's leading shape; start rows from `rng` (or RandomState(seed))."""
        lead = tuple(feat_map.shape[:-1])
        n = int(np.prod(lead))
        rng = rng if rng is not None else np.random.RandomState(seed)
        rows = kmeans_start_rows(n, int(num_clusters), int(num_init), rng)
        return self.kmeans(feat_map, num_clusters, init_rows=rows)["labels"].reshape(lead)

    # ---- canvas -----------------------------------------------------------------------------------
    def new_canvas(self, height: int, width: int, color=(1.0, 1.0, 1.0)) -> torch.Tensor:
        """A canvas fp32 [3, height, width] filled with one colour (kept as self.canvas)."""
        self.canvas = self._new((3, int(height), int(width)))
        self.fill((0, 0, int(height), int(width)), color)
        return self.canvas

    def _rect(self, rect):
        y0, x0, H, W = (int(v) for v in rect)
        cv = self.canvas
        if cv is None:
            raise _lib.DvtError("no canvas: call new_canvas first")
        return cv.data_ptr(), cv.shape[1], cv.shape[2], y0, x0, H, W

    def fill(self, rect, color=(1.0, 1.0, 1.0)) -> None:
        cv, ch, cw, y0, x0, H, W = self._rect(rect)
        _lib.check(_lib.lib().dvt_vis_fill(cv, ch, cw, y0, x0, H, W, float(color[0]), float(color[1]), float(color[2]),
                                           _lib.stream()), "dvt_vis_fill")

    def render_scalar(self, smap: torch.Tensor, rect, cmap: str | torch.Tensor | None = None, interp: str = "nearest",
                      neg_red: bool = False) -> None:
        """A scalar map [h, w] into rect = (y0, x0, H, W) of the canvas, through a colour table (name or device [256, 3])."""
        _lib.require_cuda(smap)
        smap = smap.to(torch.float32).contiguous()
        if smap.dim() != 2:
            raise _lib.DvtError("render_scalar needs a map [h, w]")
        tab = self.table(cmap) if isinstance(cmap, str) else cmap
        if tab is not None:
            _lib.require_cuda(tab)
            tab = tab.to(torch.float32).contiguous()
            if tuple(tab.shape) != (256, 3):
                raise _lib.DvtError("a scalar colour table is [256, 3]")
        cv, ch, cw, y0, x0, H, W = self._rect(rect)
        _lib.check(_lib.lib().dvt_vis_render_scalar(smap.data_ptr(), smap.shape[0], smap.shape[1], INTERP[interp], _lib.ptr(tab),
                                                    int(bool(neg_red)), cv, ch, cw, y0, x0, H, W, _lib.stream()),
                   "dvt_vis_render_scalar")

    def render_rgb(self, cmap3: torch.Tensor, rect, interp: str = "nearest", planar: bool = False) -> None:
        """A colour map [h, w, 3] (planar: [3, h, w]) into rect."""
        _lib.require_cuda(cmap3)
        cmap3 = cmap3.to(torch.float32).contiguous()
        if cmap3.dim() != 3 or cmap3.shape[0 if planar else 2] != 3:
            raise _lib.DvtError("render_rgb needs [h, w, 3], or [3, h, w] with planar=True")
        h, wd = (cmap3.shape[1], cmap3.shape[2]) if planar else (cmap3.shape[0], cmap3.shape[1])
        cv, ch, cw, y0, x0, H, W = self._rect(rect)
        _lib.check(_lib.lib().dvt_vis_render_rgb(cmap3.data_ptr(), h, wd, int(bool(planar)), INTERP[interp], cv, ch, cw, y0, x0,
                                                 H, W, _lib.stream()), "dvt_vis_render_rgb")

    def render_labels(self, labels: torch.Tensor, rect, num_clusters: int, cmap: str | torch.Tensor = "rainbow") -> None:
        """Labels [h, w] into rect through a K-entry table (`plt.get_cmap(cmap, K)` or a device [K, 3])."""
        _lib.require_cuda(labels)
        labels = labels.to(torch.int32).contiguous()
        if labels.dim() != 2:
            raise _lib.DvtError("render_labels needs labels [h, w]")
        tab = self.table(cmap, num_clusters) if isinstance(cmap, str) else cmap.to(torch.float32).contiguous()
        _lib.require_cuda(tab)
        if tuple(tab.shape) != (int(num_clusters), 3):
            raise _lib.DvtError(f"the label colour table is [{num_clusters}, 3]")
        cv, ch, cw, y0, x0, H, W = self._rect(rect)
        _lib.check(_lib.lib().dvt_vis_render_labels(labels.data_ptr(), labels.shape[0], labels.shape[1], tab.data_ptr(),
                                                    int(num_clusters), cv, ch, cw, y0, x0, H, W, _lib.stream()),
                   "dvt_vis_render_labels")

    def canvas_u8(self, out: torch.Tensor | None = None) -> torch.Tensor:
        """The canvas as uint8 [H, W, 3] on the device ((canvas * 255) truncated)."""
        cv = self.canvas
        if cv is None:
            raise _lib.DvtError("no canvas: call new_canvas first")
        if out is None:
            out = self._new((cv.shape[1], cv.shape[2], 3), torch.uint8)
        _lib.check(_lib.lib().dvt_vis_canvas_to_u8(cv.data_ptr(), cv.shape[1], cv.shape[2], out.data_ptr(), _lib.stream()),
                   "dvt_vis_canvas_to_u8")
        return out
