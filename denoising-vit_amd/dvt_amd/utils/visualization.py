"""The reference's `dvt.utils.visualization` names on the HIP kernels of `dvt_amd.vis`.

`get_robust_pca`, `get_pca_map`, `get_scale_map`, `get_similarity_map`, `get_cluster_map`,
`visualize_offline_denoised_samples` and `visualize_online_denoised_samples` take the reference's arguments and return the
reference's shapes, so code written against `dvt.utils.visualization` runs.  What differs, on purpose:

* the PCA basis is deterministic (orthogonal iteration from a fixed start, largest component of each direction positive)
  where `torch.pca_lowrank` is randomised and defined up to sign;
* `get_cluster_map` takes a `seed` (its start rows come from `numpy.random.RandomState(seed)`, the kernels draw nothing);
* a tile is composed on the device: `hcat` / `vcat` / `add_border` / `add_label` of the reference's layout helpers are
  re-expressed as canvas geometry (`tile_geometry`, a pure host function that returns every panel's rectangle), each panel
  is rendered straight into its rectangle, and the finished uint8 picture leaves the device in one copy;
* labels are drawn on the host with PIL's built-in font at size 58 unless a TrueType file is given (`font=`).
"""
from __future__ import annotations

from string import ascii_letters, digits, punctuation

import numpy as np
import torch

from .. import _lib
from ..vis import VisEngine

OFFLINE_LABELS = ("Input Image", "Original Feature", "Original Cluster", "Original Norm", "Original Sim",
                  "Denoised Feat (F)", "Denoised Cluster", "Denoised Norm", "Denoised Sim", "Shared Noise (G)",
                  "Residual Norm (h)", "Composited (G+h)")
ONLINE_LABELS = ("Input Image", "Original Feature", "Original Norm", "GT Denoised", "GT Denoised Norm", "Pred Denoised",
                 "Pred Deno. Norm")
FEATURE_LABELS = ("Input Image", "Original Feature", "Original Cluster", "Original Norm", "Original Sim",
                  "Denoised Feat (F)", "Denoised Cluster", "Denoised Norm", "Denoised Sim")
LABEL_FONT_SIZE = 58
PANEL_GAP = 12   # hcat(..., gap=12) of a row
ROW_GAP = 8      # vcat's default gap between the rows
LABEL_GAP = 4    # add_label: vcat(label, image, gap=4)
BORDER = 8       # add_border's default
_EXPECTED_CHARACTERS = digits + punctuation + ascii_letters

_engines: dict = {}


def engine_for(device) -> VisEngine:
    """One VisEngine per device for the stand-alone functions (the drivers own theirs)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.DvtError("the visualisation needs HIP device tensors; there is no CPU fallback")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _engines:
        _engines[device] = VisEngine(device)
    return _engines[device]


# ================================================================================================ pure host pieces
def tile_geometry(rows, label_sizes=None, gap: int = PANEL_GAP, row_gap: int = ROW_GAP, label_gap: int = LABEL_GAP,
                  border: int = BORDER) -> dict:
    """Where everything lands in `add_border(vcat(hcat(row 0 with add_label), hcat(row 1), ...))`.

    rows: per row the (height, width) of each panel; label_sizes: the (height, width) of the first row's labels, or None.
    A labelled cell is the label over the panel (gap `label_gap`), both centred in a cell as wide as the wider of the two;
    a row puts its cells side by side from the top (gap `gap`); rows stack from the left (gap `row_gap`); `border` pixels
    surround the whole.  Returns {"height", "width", "panels": [[(y0, x0, h, w), ...], ...], "labels": [(y0, x0, h, w), ...]}."""
    panels, labels, y, width = [], [], border, 0
    for r, row in enumerate(rows):
        x, row_h, rects = border, 0, []
        for i, (h, w) in enumerate(row):
            h, w = int(h), int(w)
            if i > 0:
                x += gap
            if r == 0 and label_sizes is not None:
                lh, lw = (int(v) for v in label_sizes[i])
                cell_w = max(lw, w)
                labels.append((y, x + (cell_w - lw) // 2, lh, lw))
                rects.append((y + lh + label_gap, x + (cell_w - w) // 2, h, w))
                cell_h = lh + label_gap + h
            else:
                cell_w, cell_h = w, h
                rects.append((y, x, h, w))
            x += cell_w
            row_h = max(row_h, cell_h)
        panels.append(rects)
        width = max(width, x - border)
        y += row_h + (row_gap if r + 1 < len(rows) else 0)
    return {"height": y + border, "width": width + 2 * border, "panels": panels, "labels": labels}


def load_font(font=None, font_size: int = LABEL_FONT_SIZE):
    from PIL import ImageFont
    if font is not None:
        return ImageFont.truetype(str(font), font_size)
    return ImageFont.load_default(size=font_size)


def draw_label(text: str, font=None, font_size: int = LABEL_FONT_SIZE) -> np.ndarray:
    """A black label on white, float32 [3, height, width]: as wide as the text, as high as the font's full character set."""
    from PIL import Image, ImageDraw
    f = load_font(font, font_size)
    left, _, right, _ = f.getbbox(text)
    _, top, _, bottom = f.getbbox(_EXPECTED_CHARACTERS)
    image = Image.new("RGB", (max(1, int(right - left)), max(1, int(bottom - top))), color="white")
    ImageDraw.Draw(image).text((0, 0), text, font=f, fill="black")
    return np.ascontiguousarray((np.asarray(image) / 255).astype(np.float32).transpose(2, 0, 1))


_label_cache: dict = {}


def _labels(texts, font, font_size=LABEL_FONT_SIZE):
    key = (tuple(texts), None if font is None else str(font), font_size)
    if key not in _label_cache:
        _label_cache[key] = [draw_label(t, font, font_size) for t in texts]
    return _label_cache[key]


def view_indices(num_views: int, num_vis_samples: int, seed: int) -> np.ndarray:
    """The views a stage-1 tile shows: `num_vis_samples` random ones plus the original image (the last view), drawn from a
    generator of their own -- the global numpy stream belongs to the fit's index draws."""
    rng = np.random.RandomState(seed)
    return np.append(rng.randint(0, num_views, size=num_vis_samples), num_views).astype(np.int64)


def save_image(path: str, picture: np.ndarray) -> None:
    """Write a uint8 [H, W, 3] picture (format by extension; names without a known one become .png)."""
    import os
    from PIL import Image
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if os.path.splitext(path)[1].lower() not in (".png", ".jpg", ".jpeg", ".bmp", ".webp"):
        path += ".png"
    Image.fromarray(np.ascontiguousarray(picture)).save(path)


# ================================================================================================ the reference's functions
def _map3(feat_map: torch.Tensor) -> torch.Tensor:
    """[1, h, w, C] or [h, w, C] -> [h, w, C]."""
    if feat_map.dim() == 4 and feat_map.shape[0] == 1:
        feat_map = feat_map[0]
    if feat_map.dim() != 3:
        raise _lib.DvtError(f"a feature map is [h, w, C] or [1, h, w, C], not {tuple(feat_map.shape)}")
    return feat_map


def _panel_to_numpy(eng: VisEngine) -> np.ndarray:
    return eng.canvas.permute(1, 2, 0).cpu().numpy()


def get_robust_pca(features: torch.Tensor, m: float = 2, remove_first_component: bool = False):
    """features [N, C] -> (reduction_mat [C, 3], rgb_min [3], rgb_max [3]), device tensors."""
    assert len(features.shape) == 2, "features should be (N, C)"
    _lib.require_cuda(features)
    return engine_for(features.device).robust_pca(features, m, remove_first_component)


def get_pca_map(feat_map, img_size, interp="nearest", return_pca_stats=False, pca_stats=None, engine: VisEngine | None = None):
    _lib.require_cuda(feat_map)
    eng = engine or engine_for(feat_map.device)
    colors, stats = eng.pca_map(_map3(feat_map), pca_stats)
    eng.new_canvas(img_size[0], img_size[1])
    eng.render_rgb(colors, (0, 0, img_size[0], img_size[1]), interp)
    out = _panel_to_numpy(eng)
    return (out, stats) if return_pca_stats else out


def get_scale_map(scalar_map, img_size, interp="nearest", engine: VisEngine | None = None):
    _lib.require_cuda(scalar_map)
    eng = engine or engine_for(scalar_map.device)
    eng.new_canvas(img_size[0], img_size[1])
    eng.render_scalar(eng.scale_map(_map3(scalar_map)), (0, 0, img_size[0], img_size[1]), "inferno", interp)
    return _panel_to_numpy(eng)


def get_similarity_map(features: torch.Tensor, img_size=(224, 224), engine: VisEngine | None = None):
    assert len(features.shape) == 4, "features should be (1, H, W, C)"
    _lib.require_cuda(features)
    eng = engine or engine_for(features.device)
    eng.new_canvas(img_size[0], img_size[1])
    eng.render_scalar(eng.similarity_map(features), (0, 0, img_size[0], img_size[1]), "turbo", "bilinear", neg_red=True)
    return _panel_to_numpy(eng)


def get_cluster_map(feat_map, img_size, num_clusters=10, seed: int = 0, engine: VisEngine | None = None):
    _lib.require_cuda(feat_map)
    eng = engine or engine_for(feat_map.device)
    labels = eng.cluster_map(_map3(feat_map), num_clusters, seed=seed)
    eng.new_canvas(img_size[0], img_size[1])
    eng.render_labels(labels, (0, 0, img_size[0], img_size[1]), num_clusters)
    return _panel_to_numpy(eng)


# ================================================================================================ tiles
class _Tile:
    """A tile under construction: geometry, canvas and the cursor of the row being rendered."""

    def __init__(self, eng: VisEngine, n_rows: int, n_cols: int, hw, label_texts, font):
        self.eng = eng
        labels = _labels(label_texts, font)
        self.geo = tile_geometry([[tuple(hw)] * n_cols] * n_rows, [lab.shape[1:] for lab in labels])
        eng.new_canvas(self.geo["height"], self.geo["width"])
        cache = eng._label_bitmaps  # on the device once per engine
        for text, lab, rect in zip(label_texts, labels, self.geo["labels"]):
            key = (text, None if font is None else str(font))
            if key not in cache:
                cache[key] = eng.upload(lab)
            eng.render_rgb(cache[key], rect, planar=True)

    def rect(self, row: int, col: int):
        return self.geo["panels"][row][col]


def _feature_panels(eng: VisEngine, tile: _Tile, row: int, col: int, feats: torch.Tensor, rng, num_clusters: int = 5):
    """PCA / cluster / norm / similarity of one map into four consecutive cells."""
    fm = _map3(feats)
    eng.render_rgb(eng.pca_map(fm)[0], tile.rect(row, col))
    eng.render_labels(eng.cluster_map(fm, num_clusters, rng=rng), tile.rect(row, col + 1), num_clusters)
    eng.render_scalar(eng.scale_map(fm), tile.rect(row, col + 2), "inferno")
    eng.render_scalar(eng.similarity_map(fm), tile.rect(row, col + 3), "turbo", "bilinear", neg_red=True)


def _image_panel(eng: VisEngine, tile: _Tile, row: int, img: torch.Tensor, denormalizer):
    img = img.to(eng.device)
    if denormalizer is not None:
        img = denormalizer(img)
    img = img.reshape(3, img.shape[-2], img.shape[-1]).float()
    eng.render_rgb(img, tile.rect(row, 0), planar=True)


def compose_offline_tile(denoiser, neural_field, raw_features, coord, patch_images, device, denormalizer=None, font=None,
                         seed: int = 0, engine: VisEngine | None = None):
    """The stage-1 tile on the device: (uint8 [H, W, 3] device tensor, the last sample's forward outputs, geometry).
    Everything is enqueued on the current stream; host arrays go up through pinned memory, so the host does not wait for
    the stream (inputs given as CPU tensors are the exception: hand over device tensors)."""
    eng = engine or engine_for(device)
    rng = np.random.RandomState(seed)
    n = len(raw_features)
    hw = tuple(patch_images.shape[-2:])
    residual = bool(getattr(denoiser, "use_residual_predictor", False))
    texts = OFFLINE_LABELS if residual else OFFLINE_LABELS[:10]
    tile = _Tile(eng, n, len(texts), hw, texts, font)
    output = None
    for i in range(n):
        with torch.no_grad():
            output = denoiser.forward(raw_vit_outputs=raw_features[i:i + 1].to(eng.device),
                                      global_pixel_coords=coord[i:i + 1].to(eng.device), neural_field=neural_field,
                                      return_visualization=True)
        _image_panel(eng, tile, i, patch_images[i:i + 1], denormalizer)
        _feature_panels(eng, tile, i, 1, output["raw_vit_outputs"].float(), rng)
        _feature_panels(eng, tile, i, 5, output["denoised_feats"].float(), rng)
        eng.render_rgb(eng.pca_map(_map3(output["shared_patterns"].float()))[0], tile.rect(i, 9))
        if "pred_residual" in output:
            eng.render_scalar(eng.scale_map(_map3(output["pred_residual"].float())), tile.rect(i, 10), "inferno")
            eng.render_rgb(eng.pca_map(_map3(output["shared_patterns_and_residual"].float()))[0], tile.rect(i, 11))
    return eng.canvas_u8(), output, tile.geo


def visualize_offline_denoised_samples(denoiser, neural_field, raw_features, coord, patch_images,
                                       device=torch.device("cuda"), denormalizer=None, dtype=torch.float32, font=None,
                                       seed: int = 0, engine: VisEngine | None = None):
    """One row per sample (input crop; PCA / cluster / norm / similarity of the raw and of the denoised features; G; |h|;
    G + h), labels over the first row.  Returns (uint8 [H, W, 3], the last sample's denoised_feats as numpy)."""
    if dtype != torch.float32:
        raise _lib.DvtError("the visualisation forward runs in float32")
    picture, output, _ = compose_offline_tile(denoiser, neural_field, raw_features, coord, patch_images, device, denormalizer,
                                              font, seed, engine)
    return picture.cpu().numpy(), output["denoised_feats"].detach().float().cpu().numpy()


def visualize_online_denoised_samples(data_dict: dict, pred_denoised_feats: torch.Tensor, denormalizer=None,
                                      num_samples: int = 5, font=None, engine: VisEngine | None = None):
    """The stage-2 tile: input, raw PCA / norm, ground-truth denoised PCA / norm, and the prediction coloured with the
    ground truth's pca_stats / its norm.  Returns uint8 [H, W, 3]."""
    _lib.require_cuda(pred_denoised_feats)
    eng = engine or engine_for(pred_denoised_feats.device)
    hw = tuple(data_dict["image"].shape[-2:])
    tile = _Tile(eng, num_samples, len(ONLINE_LABELS), hw, ONLINE_LABELS, font)
    for i in range(num_samples):
        _image_panel(eng, tile, i, data_dict["image"][i], denormalizer)
        original = _map3(data_dict["original_feats"][i].float().to(eng.device))
        gt = _map3(data_dict["denoised_feats"][i].float().to(eng.device))
        pred = _map3(pred_denoised_feats[i].float())
        eng.render_rgb(eng.pca_map(original)[0], tile.rect(i, 1))
        eng.render_scalar(eng.scale_map(original), tile.rect(i, 2), "inferno")
        gt_colors, stats = eng.pca_map(gt)
        eng.render_rgb(gt_colors, tile.rect(i, 3))
        eng.render_scalar(eng.scale_map(gt), tile.rect(i, 4), "inferno")
        eng.render_rgb(eng.pca_map(pred, stats)[0], tile.rect(i, 5))
        eng.render_scalar(eng.scale_map(pred), tile.rect(i, 6), "inferno")
    return eng.canvas_u8().cpu().numpy()


def compose_feature_row(eng: VisEngine, raw: torch.Tensor, denoised: torch.Tensor, hw, image: torch.Tensor | None = None,
                        num_clusters: int = 5, seed: int = 0, font=None):
    """`python -m dvt_amd.visualize`: one labelled row from a saved raw / denoised pair (input image first when given;
    image float [3, H, W] in [0, 1]).  Returns (uint8 [H, W, 3] device tensor, geometry)."""
    texts = FEATURE_LABELS if image is not None else FEATURE_LABELS[1:]
    tile = _Tile(eng, 1, len(texts), hw, texts, font)
    rng = np.random.RandomState(seed)
    col = 0
    if image is not None:
        eng.render_rgb(image.to(eng.device).float(), tile.rect(0, 0), "bilinear", planar=True)
        col = 1
    _feature_panels(eng, tile, 0, col, raw, rng, num_clusters)
    _feature_panels(eng, tile, 0, col + 4, denoised, rng, num_clusters)
    return eng.canvas_u8(), tile.geo
