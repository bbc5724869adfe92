"""GPU: the visualisation end to end -- the stage-1 tile of a small fitted denoiser against tests/vis_reference.py panel by
panel, `stage1.main --save_vis`, and `python -m dvt_amd.visualize` over that run's outputs."""
import os
import warnings

import numpy as np
import pytest
import torch

from tests import vis_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODEL = "vit_base_patch14_dinov2.lvd142m"


def _make_image(path, h=300, w=400, k=0):
    from PIL import Image
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 255 / w), (yy * 255 / h), ((xx // (20 + 3 * k) + yy // 20) % 2) * 200], -1).astype(np.uint8)
    Image.fromarray(img).save(path)


def test_offline_tile_panel_by_panel(built_lib):
    """A small fitted denoiser (the shapes of smoke()): the tile has exactly the size the geometry function predicts, and
    every panel region, re-computed through the float64 reference from the same forward outputs (PCA basis taken from the
    GPU, so that sign and near-degenerate directions do not enter), differs by at most one grey level."""
    from dvt_amd.fit import FitEngine, FitSettings
    from dvt_amd.models import NeuralFeatureField, SingleImageDenoiser
    from dvt_amd.utils import visualization as VZ
    from dvt_amd.vis import VisEngine, color_table, kmeans_start_rows
    dev = torch.device(DEV)
    torch.manual_seed(0)
    V, H, W, C, B, T = 5, 6, 6, 64, 128, 24
    xy = torch.rand(V, H, W, 2)
    feats = torch.sin(xy.sum(-1, keepdim=True) * torch.arange(1, C + 1) * 0.3) + torch.randn(1, H, W, C) * 0.3
    s = FitSettings(feat_dim=C, noise_map_height=H, noise_map_width=W, log2_hashmap_size=12, num_iters=T, warmup_iters=3,
                    pixel_bsz=B)
    fit = FitEngine(s, V * H * W, dev)
    fit.reset(torch.Generator(device=dev).manual_seed(0))
    idx = np.random.RandomState(0).randint(0, V * H * W, (T, B)).astype(np.int32)
    fit.fit(feats.reshape(-1, C).to(dev), xy.reshape(-1, 2).to(dev), idx, log_every=0)
    den = SingleImageDenoiser(H, W, C).to(dev)
    field = NeuralFeatureField(feat_dim=C, n_levels=16, max_resolution=1024, log2_hashmap_size=12).to(dev)
    den.start_residual_predictor()
    fit.export_modules(den, field)
    hw = (32, 32)
    images = torch.rand(V, 3, *hw)
    eng = VisEngine(dev, max_rows=H * W, max_channels=C, max_clusters=5)
    n_rows, seed = 3, 11
    picture, last = VZ.visualize_offline_denoised_samples(den, field, feats[:n_rows].to(dev), xy[:n_rows].to(dev),
                                                          images[:n_rows], dev, denormalizer=None, seed=seed, engine=eng)
    sizes = [VZ.draw_label(t).shape[1:] for t in VZ.OFFLINE_LABELS]
    geo = VZ.tile_geometry([[hw] * 12] * n_rows, sizes)
    assert picture.dtype == np.uint8 and picture.shape == (geo["height"], geo["width"], 3)
    assert last.shape == (1, H, W, C)
    # white outside every rectangle
    inside = np.zeros(picture.shape[:2], bool)
    for y, x, h, w in [p for row in geo["panels"] for p in row] + geo["labels"]:
        inside[y:y + h, x:x + w] = True
    assert (picture[~inside] == 255).all()
    for (y, x, h, w), lab in zip(geo["labels"], [VZ.draw_label(t) for t in VZ.OFFLINE_LABELS]):
        assert np.array_equal(picture[y:y + h, x:x + w], R.to_u8(lab.transpose(1, 2, 0)))

    inferno, turbo, rainbow = color_table("inferno"), color_table("turbo"), color_table("rainbow", 5)
    rng = np.random.RandomState(seed)
    worst = 0

    def check(row, col, want_rgb):
        nonlocal worst
        y, x, h, w = geo["panels"][row][col]
        d = np.abs(picture[y:y + h, x:x + w].astype(np.int32) - R.to_u8(want_rgb).astype(np.int32)).max()
        worst = max(worst, int(d))
        assert d <= 1, (row, col, d)

    def pca_panel(x64):
        basis, _ = eng.pca_basis(torch.from_numpy(x64).to(dev))  # the GPU's basis; range and colours in float64
        b = basis.cpu().numpy()
        r = R.robust_range(x64.reshape(-1, C) @ b.astype(np.float64))
        return R.resample(R.pca_colors(x64, b, r["rgb_min"].astype(np.float32), r["rgb_max"].astype(np.float32)), hw)

    def four(row, col, x64):
        check(row, col, pca_panel(x64))
        starts = kmeans_start_rows(H * W, 5, 8, rng)
        km = R.kmeans(x64.reshape(-1, C), x64.reshape(-1, C)[starts])
        check(row, col + 1, R.labels_panel(km["labels"].reshape(H, W), hw, rainbow))
        check(row, col + 2, R.scalar_panel(R.scale_map(x64), hw, inferno))
        check(row, col + 3, R.scalar_panel(R.similarity_map(x64), hw, turbo, "bilinear", neg_red=True))

    for i in range(n_rows):
        with torch.no_grad():
            out = den.forward(raw_vit_outputs=feats[i:i + 1].to(dev), global_pixel_coords=xy[i:i + 1].to(dev),
                              neural_field=field, return_visualization=True)
        out = {k: v.float().cpu().numpy().astype(np.float64) for k, v in out.items() if v.dim() == 4}
        check(i, 0, images[i].numpy().transpose(1, 2, 0))
        four(i, 1, out["raw_vit_outputs"][0])
        four(i, 5, out["denoised_feats"][0])
        check(i, 9, pca_panel(out["shared_patterns"][0]))
        check(i, 10, R.scalar_panel(R.scale_map(out["pred_residual"][0]), hw, inferno))
        check(i, 11, pca_panel(out["shared_patterns_and_residual"][0]))
    print("offline tile: worst panel difference", worst, "grey levels")


def _run_stage1(tmp_path, tag, extra):
    from dvt_amd import stage1
    argv = ["--img_path", str(tmp_path / "list.txt"), "--data_root", str(tmp_path / "data"), "--save_root",
            str(tmp_path / tag), "--output_dir", str(tmp_path / (tag + "_work")), "--num_views", "15", "--num_iters", "40",
            "--warmup_iters", "4", "--pixel_bsz", "512", "--num_imgs", "10", "--allow_random_vit", "--dtype", "bfloat16"] + extra
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # random ViT weights (no checkpoint offline)
        assert stage1.main(stage1.get_args(argv)) == 3
    out = {}
    for rel in ("sub/a.npy", "b.npy", "c.npy"):
        out[rel] = (np.load(tmp_path / tag / "raw_features" / MODEL / rel), np.load(tmp_path / tag / "denoised_features" / MODEL / rel))
    return out


def test_stage1_save_vis_and_visualize(built_lib, tmp_path):
    """`stage1.main --save_vis --vis_freq 1 --num_vis_samples 2` on three images writes three pictures of the predicted
    size and leaves the saved features as they are without the flag.

    Run-to-run spread of the unchanged command, established first by running it twice: measured 0 (raw and denoised
    features of two plain runs are bit-identical on an MI355X at this configuration), so the --save_vis run has to be
    bit-identical too.  The spread is measured again on every run and is the only distance allowed."""
    from PIL import Image
    from dvt_amd import visualize
    from dvt_amd.utils import visualization as VZ
    data_root = tmp_path / "data"
    (data_root / "sub").mkdir(parents=True)
    for k, name in enumerate(("sub/a.png", "b.png", "c.png")):
        _make_image(str(data_root / name), k=k)
    (tmp_path / "list.txt").write_text("sub/a.png\nb.png\nc.png\n")
    plain1 = _run_stage1(tmp_path, "plain1", [])
    plain2 = _run_stage1(tmp_path, "plain2", [])
    vis = _run_stage1(tmp_path, "vis", ["--save_vis", "--vis_freq", "1", "--num_vis_samples", "2"])
    spread = 0.0
    for rel in plain1:
        assert np.array_equal(plain1[rel][0], plain2[rel][0]) and np.array_equal(plain1[rel][0], vis[rel][0])
        spread = max(spread, float(np.abs(plain1[rel][1] - plain2[rel][1]).max()))
    worst = 0.0
    for rel in plain1:
        d = min(float(np.abs(vis[rel][1] - plain1[rel][1]).max()), float(np.abs(vis[rel][1] - plain2[rel][1]).max()))
        worst = max(worst, d)
    print(f"stage-1 run-to-run spread of the denoised features {spread:.3e}; --save_vis run differs by {worst:.3e}")
    assert worst <= spread
    sizes = [VZ.draw_label(t).shape[1:] for t in VZ.OFFLINE_LABELS]
    geo = VZ.tile_geometry([[(518, 518)] * 12] * 3, sizes)
    vis_dir = tmp_path / "vis_work" / "visualization"
    assert sorted(os.listdir(vis_dir)) == ["a.png", "b.png", "c.png"]
    for name in ("a.png", "b.png", "c.png"):
        with Image.open(vis_dir / name) as im:
            assert im.size == (geo["width"], geo["height"])
            a = np.asarray(im.convert("RGB"))
        y, x, h, w = geo["panels"][1][3]
        assert (a[:8] == 255).all() and a[y:y + h, x:x + w].std() > 0
    assert not os.path.isdir(tmp_path / "plain1_work" / "visualization")

    # python -m dvt_amd.visualize over that run's save_root: one picture per image, one column more with --data_root
    for with_images in (False, True):
        out_dir = tmp_path / ("rows_img" if with_images else "rows")
        argv = ["--save_root", str(tmp_path / "vis"), "--model", MODEL, "--output_dir", str(out_dir)]
        if with_images:
            argv += ["--data_root", str(data_root), "--img_path", str(tmp_path / "list.txt")]
        assert visualize.main(visualize.get_args(argv), device=torch.device(DEV)) == 3
        n_cols = 9 if with_images else 8
        labels = VZ.FEATURE_LABELS if with_images else VZ.FEATURE_LABELS[1:]
        g = VZ.tile_geometry([[(518, 518)] * n_cols], [VZ.draw_label(t).shape[1:] for t in labels])
        for rel in ("sub/a.png", "b.png", "c.png"):
            with Image.open(out_dir / rel) as im:
                assert im.size == (g["width"], g["height"])
