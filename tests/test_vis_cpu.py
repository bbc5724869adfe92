"""CPU: the float64 reference of the visualisation (tests/vis_reference.py) reproduces what the reference's functions
returned on the committed fixtures (tests/golden/vis_reference.npz, recorded by make_vis_golden.py), the colour-table rule
is matplotlib's, and the host logic of the tile, of `--save_vis` and of `python -m dvt_amd.visualize` is right."""
import json
import os

import numpy as np
import pytest
import torch

from tests import vis_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("planted", "odd", "zero_dev", "duplicates")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "vis_reference.npz")), json.load(open(os.path.join(GOLDEN, "vis_reference.json")))


def test_fixtures_are_small_and_cover_the_cases(gold):
    arrays, meta = gold
    assert os.path.getsize(os.path.join(GOLDEN, "vis_reference.npz")) < 1 << 20
    shapes = {n: arrays[f"{n}.x"].shape for n in FIXTURES}
    assert all(s[0] <= 16 and s[1] <= 16 and s[2] <= 128 for s in shapes.values())
    assert (shapes["planted"][0] * shapes["planted"][1]) % 2 == 0 and (shapes["odd"][0] * shapes["odd"][1]) % 2 == 1
    ev = meta["planted_eigenvalues"]  # well separated leading directions
    assert ev[0] / ev[1] > 2.5 and ev[1] / ev[2] > 2.5
    assert 0 < meta["e_pca"] < 1e-6 and 0 < meta["e_map"] < 1e-5
    assert "not recorded" in meta["get_cluster_map"]


@pytest.mark.parametrize("name", FIXTURES)
def test_robust_range_for_a_given_basis(gold, name):
    arrays, _ = gold
    x, basis = arrays[f"{name}.x"], arrays[f"{name}.basis"]
    colors = (torch.from_numpy(x).reshape(-1, x.shape[-1]) @ torch.from_numpy(basis)).numpy()  # the reference's fp32 product
    got = R.robust_range(colors)
    assert np.array_equal(got["rgb_min"].astype(np.float32), arrays[f"{name}.rgb_min"])
    assert np.array_equal(got["rgb_max"].astype(np.float32), arrays[f"{name}.rgb_max"])
    assert got["rows"][12] == (1 if name == "zero_dev" else 0)
    if name == "zero_dev":
        assert got["deviation"][0] == 0.0 and len(set(got["rgb_min"])) == 1 and len(set(got["rgb_max"])) == 1


@pytest.mark.parametrize("name", FIXTURES)
def test_maps_reproduce_the_recorded_arrays(gold, name):
    arrays, meta = gold
    size = tuple(meta["size"])
    x = arrays[f"{name}.x"]
    pca = R.resample(R.pca_colors(x, arrays[f"{name}.basis"], arrays[f"{name}.rgb_min"], arrays[f"{name}.rgb_max"]), size)
    assert np.abs(pca - arrays[f"{name}.pca_map"]).max() <= 1e-6
    scale = R.resample(R.scale_map(x), size)
    assert np.abs(scale - arrays[f"{name}.scale_float"]).max() <= 1e-6
    sim = R.resample(R.similarity_map(x), size, "bilinear")
    assert np.abs(sim - arrays[f"{name}.sim_float"]).max() <= 1e-6


@pytest.mark.parametrize("name", FIXTURES)
def test_colour_tables_are_matplotlibs(gold, name):
    """Exact, except where the float64 value and the recorded fp32 value sit on different sides of a table boundary: then
    at most one table step."""
    from dvt_amd.vis import color_table
    arrays, meta = gold
    size = tuple(meta["size"])
    x = arrays[f"{name}.x"]
    for key, smap, cmap, interp in (("scale", R.scale_map(x), "inferno", "nearest"), ("sim", R.similarity_map(x), "turbo", "bilinear")):
        table = color_table(cmap)
        v64, v32 = R.resample(smap, size, interp), arrays[f"{name}.{key}_float"]
        # the rule itself, on the recorded floats: exact
        want = arrays[f"{name}.{key}_rgb"]
        got = R.apply_table(v32, table)
        if key == "sim":
            got[v32 < 0] = (1.0, 0.0, 0.0)
        assert np.array_equal(got.astype(np.float32), want)
        # through the float64 values: at most one step, and only on a boundary
        i64, i32 = R.table_index(v64), R.table_index(v32)
        assert np.abs(i64 - i32).max() <= 1
        same = i64 == i32
        panel = R.scalar_panel(smap, size, table, interp, neg_red=(key == "sim"))
        assert np.array_equal(panel[same].astype(np.float32), want[same])


def test_label_table_is_get_cmap_with_k_entries():
    import matplotlib.pyplot as plt
    from dvt_amd.vis import color_table
    for k in (5, 10):
        labels = np.arange(k)
        assert np.array_equal(color_table("rainbow", k), plt.get_cmap("rainbow", k)(labels)[:, :3].astype(np.float32))
    v = np.linspace(0, 1, 1001).astype(np.float32)
    assert np.array_equal(R.apply_table(v, color_table("inferno")).astype(np.float32),
                          plt.get_cmap("inferno")(v)[:, :3].astype(np.float32))


@pytest.mark.parametrize("case", ["offline_tile", "online_tile"])
def test_tile_geometry_is_the_references(gold, case):
    from dvt_amd.utils.visualization import tile_geometry
    rec = gold[1][case]
    n_cols = len(rec["labels"])
    geo = tile_geometry([[tuple(rec["hw"])] * n_cols] * rec["rows"], [tuple(s) for s in rec["label_sizes"]])
    assert (geo["height"], geo["width"]) == (rec["height"], rec["width"])
    assert [[list(p) for p in row] for row in geo["panels"]] == rec["panels"]


def test_tile_geometry_of_the_stage1_case():
    """518 x 518 panels, 12 columns, 6 rows (num_vis_samples 5 + the original), labels narrower than the panels."""
    from dvt_amd.utils.visualization import OFFLINE_LABELS, draw_label, tile_geometry
    sizes = [draw_label(t).shape[1:] for t in OFFLINE_LABELS]
    lh = sizes[0][0]
    assert all(s[0] == lh and s[1] <= 518 for s in sizes)
    geo = tile_geometry([[(518, 518)] * 12] * 6, sizes)
    assert geo["width"] == 12 * 518 + 11 * 12 + 16
    assert geo["height"] == 6 * 518 + (lh + 4) + 5 * 8 + 16
    assert geo["panels"][0][0] == (8 + lh + 4, 8, 518, 518) and geo["panels"][5][11] == (geo["height"] - 8 - 518, geo["width"] - 8 - 518, 518, 518)
    for (y, x, h, w), s in zip(geo["labels"], sizes):
        assert y == 8 and (h, w) == tuple(s)
    flat = [p for row in geo["panels"] for p in row] + geo["labels"]
    for y, x, h, w in flat:  # inside the canvas, and no two rectangles overlap
        assert 0 <= y and y + h <= geo["height"] and 0 <= x and x + w <= geo["width"]
    for i, a in enumerate(flat):
        for b in flat[i + 1:]:
            assert a[0] + a[2] <= b[0] or b[0] + b[2] <= a[0] or a[1] + a[3] <= b[1] or b[1] + b[3] <= a[1]


def test_view_indices_leave_the_global_numpy_stream_alone():
    from dvt_amd.utils.visualization import view_indices
    np.random.seed(3)
    before = np.random.get_state()
    idx = view_indices(768, 5, seed=17)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert idx.shape == (6,) and idx[-1] == 768 and ((0 <= idx[:-1]) & (idx[:-1] < 768)).all()
    assert np.array_equal(idx, view_indices(768, 5, seed=17)) and not np.array_equal(idx, view_indices(768, 5, seed=18))


def test_save_vis_is_an_extra_flag_and_off_by_default():
    from dvt_amd import stage1
    a = stage1.get_args([])
    assert a.save_vis is False and a.vis_font is None and (a.num_vis_samples, a.vis_freq) == (5, 100)
    b = stage1.get_args(["--save_vis", "--vis_freq", "1", "--num_vis_samples", "2", "--vis_font", "x.ttf"])
    assert b.save_vis is True and (b.num_vis_samples, b.vis_freq, b.vis_font) == (2, 1, "x.ttf")


def test_visualize_pairs_and_shards(tmp_path):
    from dvt_amd import visualize
    from dvt_amd.utils import misc
    save_root, model = str(tmp_path / "out"), "m"
    names = [f"a/img{i}.jpg" for i in range(7)]
    for i, n in enumerate(names):
        raw_p, den_p = misc.output_paths(save_root, model, "data", os.path.join("data", n))
        if i != 3:  # image 3 has no denoised file: not a pair
            misc.atomic_save_npy(den_p, np.zeros((1, 2, 2, 64), np.float32))
        misc.atomic_save_npy(raw_p, np.zeros((2, 2, 64), np.float32))
    pairs = visualize.find_pairs(save_root, model)
    assert [p[0] for p in pairs] == [f"a/img{i}" for i in (0, 1, 2, 4, 5, 6)]
    assert all(os.path.isfile(p[1]) and os.path.isfile(p[2]) for p in pairs)
    args = visualize.get_args(["--save_root", save_root, "--model", model, "--output_dir", str(tmp_path / "vis"),
                               "--start_idx", "1", "--num_imgs", "4"])
    assert args.num_clusters == 5
    picked = visualize.select(pairs, args.start_idx, args.num_imgs)
    assert [p[0] for p in picked] == [f"a/img{i}" for i in (1, 2, 4, 5)]
    shards = [visualize.shard(picked, r, 3) for r in range(3)]
    assert sum(shards, []) == picked and all(len(s) >= 1 for s in shards)
    # the image of a pair, from a work-list as stage 1 reads it
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(n + " 0" for n in names))
    lookup = visualize.image_lookup("data", str(lst))
    assert lookup["a/img4"] == os.path.join("data", "a/img4.jpg")


def test_no_cpu_fallback():
    from dvt_amd import _lib
    from dvt_amd.utils import visualization as V
    from dvt_amd.vis import VisEngine
    with pytest.raises(_lib.DvtError):
        VisEngine("cpu")
    with pytest.raises(_lib.DvtError):
        V.get_scale_map(torch.zeros(1, 4, 4, 64), (8, 8))
    with pytest.raises(_lib.DvtError):
        V.get_robust_pca(torch.zeros(16, 64))


def test_bad_arguments_are_rejected(built_lib):
    lib = built_lib
    assert lib.dvt_vis_workspace_bytes(1369, 768, 5, 8) > 768 * 768 * 4
    assert lib.dvt_vis_workspace_bytes(1369, 100, 5, 8) == -1  # C % 64
    assert lib.dvt_vis_workspace_bytes(1369, 2048, 5, 8) == -1
    assert lib.dvt_vis_workspace_bytes(0, 768, 5, 8) == -1
    assert lib.dvt_vis_workspace_bytes(1369, 768, 17, 8) == -1
    assert lib.dvt_vis_pca_basis(None, None, 16, 64, 8, None, None, None, 0, None) == -1
    assert lib.dvt_vis_pca_basis(1, None, 16, 64, 8, 1, 1, 1, 16, None) == -1  # workspace too small
    assert lib.dvt_vis_kmeans(1, 16, 64, 0, 1, None, 1, 10, 1e-4, 1, 1, 1, 1, 1, 1, 1 << 30, None) == -1  # K = 0
    assert lib.dvt_vis_kmeans(1, 16, 64, 4, None, None, 1, 10, 1e-4, 1, 1, 1, 1, 1, 1, 1 << 30, None) == -1  # no start
    assert lib.dvt_vis_kmeans(1, 16, 64, 4, 1, None, 1, 0, 1e-4, 1, 1, 1, 1, 1, 1, 1 << 30, None) == -1  # max_iter = 0
    # rectangles outside the canvas
    for rect in ((-1, 0, 4, 4), (0, 0, 0, 4), (5, 0, 4, 4), (0, 6, 4, 3)):
        assert lib.dvt_vis_fill(1, 8, 8, *rect, 1.0, 1.0, 1.0, None) == -1
        assert lib.dvt_vis_render_scalar(1, 2, 2, 0, None, 0, 1, 8, 8, *rect, None) == -1
    assert lib.dvt_vis_render_scalar(1, 2, 2, 2, None, 0, 1, 8, 8, 0, 0, 4, 4, None) == -1  # unknown interpolation
