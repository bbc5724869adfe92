"""GPU: the public surface of `dvt_amd.utils.visualization` and the remaining VisEngine pieces against the float64 reference
in tests/vis_reference.py: the foreground mask and get_robust_pca(remove_first_component=True), every get_* function at a
small shape (result [H, W, 3], at most one grey level from the reference panel), and the stage-2 tile."""
import numpy as np
import pytest
import torch

from tests import vis_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype)


def scene(h, w, c, seed):
    """A map with a dominant 'background' direction on part of the rows (what remove_first_component is for) over a few
    smooth components and noise.  The component scales keep the leading eigenvalues apart (ratios above 1.5, asserted where
    a basis is compared): the orthogonal iteration separates direction j from j + 1 at the rate (lambda_j+1 / lambda_j)^48."""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    comps = np.stack([np.sin(3 * xx + yy), np.cos(2 * yy - xx), xx * yy], -1)
    x = comps @ (rng.standard_normal((3, c)) * np.array([4.0, 1.6, 0.6])[:, None]) + 0.3 * rng.standard_normal((h, w, c))
    bg = (xx + 0.3 * yy) > 0.8
    x[bg] += 4.0 * rng.standard_normal(c)
    return (x + rng.standard_normal(c)).astype(np.float32), bg


def planted_scene(h, w, c, seed):
    """Rows = four latent factors with scales 8, 4, 2, 1 along orthonormal directions over noise 0.1; 30 % of the rows (the
    'background') sit far out along a fifth direction.  All rows: the background direction leads; foreground rows: the
    four factors, a factor of about 4 apart."""
    rng = np.random.RandomState(seed)
    n = h * w
    q, _ = np.linalg.qr(rng.standard_normal((c, 5)))
    x = (rng.standard_normal((n, 4)) * [8.0, 4.0, 2.0, 1.0]) @ q[:, :4].T + 0.1 * rng.standard_normal((n, c))
    bg = rng.rand(n) < 0.3
    x[bg] += 60.0 * q[:, 4]
    return (x + 0.5 * rng.standard_normal(c)).reshape(h, w, c).astype(np.float32), bg


def separated(flat, mask=None, ratio=1.5):
    """The condition of the 1e-6 bound on a fitted basis: the four leading eigenvalues are a factor `ratio` apart."""
    rows = np.asarray(flat, np.float64) if mask is None else np.asarray(flat, np.float64)[mask]
    w = np.linalg.eigvalsh(np.cov(rows.T))[::-1][:4]
    return bool((w[:-1] / w[1:] > ratio).all())


def grey_levels(got, want):
    return int(np.abs(R.to_u8(got).astype(np.int32) - R.to_u8(want).astype(np.int32)).max())


@pytest.fixture(scope="module")
def eng(built_lib):
    from dvt_amd.vis import VisEngine
    return VisEngine(DEV, max_rows=37 * 37, max_channels=768, max_clusters=10)


@pytest.mark.parametrize("shape", [(16, 16, 128), (37, 37, 768)])
def test_fg_mask_and_remove_first_component(eng, shape):
    """dvt_vis_fg_mask on given colours against the reference (equal wherever the float64 value is further than 1e-6 from the
    threshold: the kernel divides in fp32, as torch does), then get_robust_pca(remove_first_component=True) end to end: the
    masked basis against float64 eigh of the masked rows, the range from the GPU's basis and mask against the reference."""
    from dvt_amd.utils import visualization as VZ
    x, _ = planted_scene(*shape, seed=3)
    flat = x.reshape(-1, shape[2])
    rng = np.random.RandomState(0)
    colors = (rng.standard_normal((flat.shape[0], 3)) * [2.0, 1.0, 0.5]).astype(np.float32)
    colors[5, 0], colors[9, 0] = colors[:, 0].min(), colors[:, 0].max()  # duplicates of the extremes
    want, value = R.fg_mask(colors, 0.2)
    got = eng.fg_mask(dev(colors), 0.2).cpu().numpy().astype(bool)
    sure = np.abs(value - 0.2) > 1e-6
    assert sure.mean() > 0.99 and np.array_equal(got[sure], want[sure]) and 0 < got.sum() < got.size
    # the pipeline: basis of all rows -> colours -> mask -> basis of the masked rows -> range over the masked rows
    basis0, _ = eng.pca_basis(dev(flat))
    assert separated(flat)
    assert (R.one_minus_abs_cos(basis0.cpu().numpy(), R.pca_basis(flat)[0]) <= 1e-6).all()
    col0 = eng.project(dev(flat), basis0).cpu().numpy()
    want_mask, value = R.fg_mask(col0, 0.2)
    mask = eng.fg_mask(dev(col0), 0.2).cpu().numpy().astype(bool)
    sure = np.abs(value - 0.2) > 1e-6
    assert np.array_equal(mask[sure], want_mask[sure]) and 0.05 * mask.size < mask.sum() < 0.95 * mask.size
    basis, lo, hi = VZ.get_robust_pca(dev(flat), remove_first_component=True)
    basis, lo, hi = basis.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()
    err = R.one_minus_abs_cos(basis, R.pca_basis(flat, mask)[0])
    assert separated(flat, mask)
    print("remove_first_component", shape, "masked rows", int(mask.sum()), "1-|cos|", err)
    assert (err <= 1e-6).all()
    col = eng.project(dev(flat), dev(basis)).cpu().numpy()
    ref = R.robust_range(col.astype(np.float64), mask, 2.0)
    assert np.array_equal(lo, ref["rgb_min"].astype(np.float32)) and np.array_equal(hi, ref["rgb_max"].astype(np.float32))
    # and without the branch: the range over all rows, on the device tensor API
    b1, lo1, hi1 = VZ.get_robust_pca(dev(flat))
    assert torch.equal(b1, basis0)
    ref1 = R.robust_range(col0.astype(np.float64), None, 2.0)
    assert np.array_equal(lo1.cpu().numpy(), ref1["rgb_min"].astype(np.float32))
    assert np.array_equal(hi1.cpu().numpy(), ref1["rgb_max"].astype(np.float32))


def test_get_functions_against_the_reference_panels(eng):
    from dvt_amd.utils import visualization as VZ
    from dvt_amd.vis import color_table, kmeans_start_rows
    h, w, c, size = 12, 10, 128, (48, 40)
    x, _ = scene(h, w, c, seed=5)
    xd = dev(x)
    # get_pca_map: fitted here (stats returned), then with the given stats, [1, h, w, C] accepted
    got, stats = VZ.get_pca_map(xd, size, return_pca_stats=True)
    b, lo, hi = (t.cpu().numpy() for t in stats)
    want = R.resample(R.pca_colors(x, b, lo, hi), size)
    assert got.shape == (*size, 3) and got.dtype == np.float32 and grey_levels(got, want) <= 1
    col = eng.project(xd, stats[0]).cpu().numpy()
    ref = R.robust_range(col.astype(np.float64))
    assert np.array_equal(lo, ref["rgb_min"].astype(np.float32)) and np.array_equal(hi, ref["rgb_max"].astype(np.float32))
    other, _ = scene(h, w, c, seed=6)
    got2 = VZ.get_pca_map(dev(other)[None], size, interp="bilinear", pca_stats=stats)
    assert got2.shape == (*size, 3) and grey_levels(got2, R.resample(R.pca_colors(other, b, lo, hi), size, "bilinear")) <= 1
    # get_scale_map / get_similarity_map
    got = VZ.get_scale_map(xd[None], size)
    assert got.shape == (*size, 3) and grey_levels(got, R.scalar_panel(R.scale_map(x), size, color_table("inferno"))) <= 1
    got = VZ.get_similarity_map(xd[None], size)
    want = R.scalar_panel(R.similarity_map(x), size, color_table("turbo"), "bilinear", neg_red=True)
    assert got.shape == (*size, 3) and grey_levels(got, want) <= 1
    assert (got[size[0] // 2 + 1, size[1] // 2 + 1] == (1.0, 0.0, 0.0)).all()  # inside the centre patch: red
    # get_cluster_map: the float64 k-means from the same start rows
    for k in (10, 5):
        got = VZ.get_cluster_map(xd, size, num_clusters=k, seed=4)
        starts = kmeans_start_rows(h * w, k, 8, np.random.RandomState(4))
        km = R.kmeans(x.reshape(-1, c), x.reshape(-1, c)[starts].astype(np.float64))
        want = R.labels_panel(km["labels"].reshape(h, w), size, color_table("rainbow", k))
        assert got.shape == (*size, 3) and grey_levels(got, want) == 0
        assert np.array_equal(got, VZ.get_cluster_map(xd, size, num_clusters=k, seed=4))


def test_online_tile(eng):
    """visualize_online_denoised_samples on a small synthetic batch: the size tile_geometry predicts, every panel against the
    reference, the prediction coloured with the GROUND TRUTH's pca_stats."""
    from dvt_amd.utils import visualization as VZ
    from dvt_amd.vis import color_table
    h, w, c, hw, n = 8, 8, 64, (40, 40), 2
    rng = np.random.RandomState(1)
    maps = {k: np.stack([scene(h, w, c, seed=10 * i + j)[0] for i in range(n)]) for j, k in enumerate(("original", "gt"))}
    pred = (maps["gt"] + 0.2 * rng.standard_normal(maps["gt"].shape)).astype(np.float32)
    images = rng.rand(n, 3, *hw).astype(np.float32)
    data = {"image": torch.from_numpy(images), "original_feats": dev(maps["original"]), "denoised_feats": dev(maps["gt"])}
    mean, std = torch.tensor([0.5, 0.4, 0.3]).view(3, 1, 1), torch.tensor([0.2, 0.25, 0.3]).view(3, 1, 1)
    picture = VZ.visualize_online_denoised_samples(data, dev(pred), denormalizer=lambda t: t * std.to(t.device) + mean.to(t.device),
                                                   num_samples=n, engine=eng)
    geo = VZ.tile_geometry([[hw] * 7] * n, [VZ.draw_label(t).shape[1:] for t in VZ.ONLINE_LABELS])
    assert picture.dtype == np.uint8 and picture.shape == (geo["height"], geo["width"], 3)
    inferno = color_table("inferno")
    worst = 0

    def check(row, col, want):
        nonlocal worst
        y, x, ph, pw = geo["panels"][row][col]
        d = int(np.abs(picture[y:y + ph, x:x + pw].astype(np.int32) - R.to_u8(want).astype(np.int32)).max())
        worst = max(worst, d)
        assert d <= 1, (row, col, d)

    def fitted(x64):
        b = eng.pca_basis(dev(x64))[0].cpu().numpy()  # the GPU's basis; range and colours in float64
        r = R.robust_range(x64.reshape(-1, c).astype(np.float64) @ b.astype(np.float64))
        return b, r["rgb_min"].astype(np.float32), r["rgb_max"].astype(np.float32)

    for i in range(n):
        check(i, 0, (images[i] * std.numpy() + mean.numpy()).transpose(1, 2, 0))
        check(i, 1, R.resample(R.pca_colors(maps["original"][i], *fitted(maps["original"][i])), hw))
        check(i, 2, R.scalar_panel(R.scale_map(maps["original"][i]), hw, inferno))
        gt_stats = fitted(maps["gt"][i])
        check(i, 3, R.resample(R.pca_colors(maps["gt"][i], *gt_stats), hw))
        check(i, 4, R.scalar_panel(R.scale_map(maps["gt"][i]), hw, inferno))
        check(i, 5, R.resample(R.pca_colors(pred[i], *gt_stats), hw))
        check(i, 6, R.scalar_panel(R.scale_map(pred[i]), hw, inferno))
        own = R.resample(R.pca_colors(pred[i], *fitted(pred[i])), hw)  # NOT its own stats: that picture differs
        y, x, ph, pw = geo["panels"][i][5]
        assert np.abs(picture[y:y + ph, x:x + pw].astype(np.int32) - R.to_u8(own).astype(np.int32)).max() > 1
    print("online tile: worst panel difference", worst, "grey levels")


def test_signed_zeros_are_one_value(eng):
    """-0.0 and +0.0 in the projected rows: one value for the selection, the lowest row that holds it is reported."""
    colors = np.zeros((9, 3), np.float32)
    colors[:, 0] = [-0.0, 0.0, 1.0, -1.0, 0.0, -0.0, 2.0, -2.0, 0.0]
    colors[:, 1] = [0.0, -0.0, 3.0, -3.0, -0.0, 0.0, 0.5, -0.5, -0.0]
    colors[:, 2] = np.arange(9)
    lo, hi, det = eng.robust_range(dev(colors), None, 2.0, details=True)
    want = R.robust_range(colors.astype(np.float64), None, 2.0)
    assert np.array_equal(det["rows"].cpu().numpy(), want["rows"])
    assert np.array_equal(lo.cpu().numpy(), want["rgb_min"].astype(np.float32))
    assert np.array_equal(hi.cpu().numpy(), want["rgb_max"].astype(np.float32))
