"""Generator of tests/golden/vis_reference.npz + vis_reference.json (run once, by hand, next to a checkout of the reference):

    python tests/golden/make_vis_golden.py /path/to/reference

It loads the reference's dvt/utils/visualization/{layout,annotation,visualization_tools}.py by file path, with stand-in
modules for what is not installed (torch_kmeans, dvt.models, jaxtyping), and records on small seeded feature maps what its
functions return: get_pca_map with given pca_stats, get_scale_map and get_similarity_map (the floats that enter the colour
table and the colours), get_robust_pca's range for a GIVEN basis (torch.pca_lowrank replaced by a function that returns
it), and the geometry of a 2-row offline and a 2-row online tile built from constant-colour panels with its hcat / vcat /
add_label / add_border.  The labels of those tiles were drawn with PIL's small bitmap fall-back font (11 px high): the
reference's add_label looks for its Inter-Regular.otf relative to the working directory and falls back when it is not
found, as here; the geometry test feeds the recorded label sizes to tile_geometry, so the font does not matter to it.
get_cluster_map cannot be recorded: torch_kmeans is not installed and not part of the
reference's tree.

It also MEASURES the reference-vs-exact spread that the GPU tolerances are built on (e_pca, e_map) and writes it into the
JSON file; tests/vis_reference.py supplies the float64 evaluation.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import vis_reference as R  # noqa: E402


def load_reference(root):
    vis_dir = os.path.join(root, "dvt", "utils", "visualization")
    for name in ("dvt", "dvt.utils", "dvt.utils.visualization", "dvt.models"):
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules.setdefault(name, mod)
    sys.modules["dvt.models"].SingleImageDenoiser = object
    sys.modules["dvt.models"].NeuralFeatureField = object
    if "torch_kmeans" not in sys.modules:
        tk = types.ModuleType("torch_kmeans")
        tk.KMeans = tk.CosineSimilarity = None
        sys.modules["torch_kmeans"] = tk
    try:
        import jaxtyping  # noqa: F401
    except ImportError:
        jt = types.ModuleType("jaxtyping")

        class _Any:
            def __class_getitem__(cls, item):
                return cls
        jt.Float = _Any
        sys.modules["jaxtyping"] = jt
    mods = {}
    for short in ("layout", "annotation", "visualization_tools"):
        full = f"dvt.utils.visualization.{short}"
        spec = importlib.util.spec_from_file_location(full, os.path.join(vis_dir, short + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[full] = mod
        spec.loader.exec_module(mod)
        mods[short] = mod
    return mods


def orthonormal(rng, rows, cols):
    q, _ = np.linalg.qr(rng.standard_normal((rows, cols)))
    return q


def fixtures():
    out = {}
    rng = np.random.RandomState(7)
    # planted spectrum, even row count (256): singular values 30, 18, 11, 6, 4, 0.5, ...
    s = np.array([30, 18, 11, 6, 4] + [0.5 * 0.9 ** i for i in range(11)])
    x = (orthonormal(rng, 256, 16) * s) @ orthonormal(rng, 128, 16).T * np.sqrt(255.0) + 0.3 * rng.standard_normal(128)
    out["planted"] = x.reshape(16, 16, 128).astype(np.float32)
    # odd row count (225), plain noise around a common direction
    out["odd"] = (rng.standard_normal((15, 15, 64)) + 2.0 * rng.standard_normal(64)).astype(np.float32)
    # a channel whose deviation is zero under the basis (e0, e1, e2): the fall-back branch
    z = rng.standard_normal((8, 8, 64))
    z.reshape(64, 64)[:40, 0] = 1.0
    out["zero_dev"] = z.astype(np.float32)
    # duplicates in the projected rows, even count
    d = rng.standard_normal((6, 6, 64))
    d.reshape(36, 64)[::2] = d.reshape(36, 64)[1::2]
    out["duplicates"] = d.astype(np.float32)
    return out


def given_basis(name, x):
    c = x.shape[-1]
    if name == "zero_dev":
        return np.eye(c, 3, dtype=np.float32)
    if name == "planted":  # near the true directions, as the stage-2 tile's pca_stats are
        return R.pca_basis(x.reshape(-1, c))[0].astype(np.float32)
    return orthonormal(np.random.RandomState(11), c, 3).astype(np.float32)


def rectangles(img, colors):
    """Bounding box (y0, x0, h, w) of each constant colour in a [3, H, W] picture."""
    out = []
    for col in colors:
        hit = np.all(np.abs(img - np.asarray(col, np.float32)[:, None, None]) < 1e-6, axis=0)
        ys, xs = np.nonzero(hit)
        out.append([int(ys.min()), int(xs.min()), int(ys.max() - ys.min() + 1), int(xs.max() - xs.min() + 1)])
    return out


def tile_case(mods, labels, n_rows, hw):
    layout, annotation = mods["layout"], mods["annotation"]
    n_cols = len(labels)
    colors = [[(0.1 + 0.8 * (r * n_cols + c) / (n_rows * n_cols - 1)), 0.25 + 0.5 * c / n_cols, 0.9 - 0.7 * r / n_rows]
              for r in range(n_rows) for c in range(n_cols)]
    rows = []
    for r in range(n_rows):
        panels = [torch.tensor(colors[r * n_cols + c], dtype=torch.float32)[:, None, None].expand(3, *hw).clone()
                  for c in range(n_cols)]
        if r == 0:
            panels = [annotation.add_label(p, t, font_size=58) for p, t in zip(panels, labels)]
        rows.append(layout.hcat(*panels, gap=12))
    tile = layout.add_border(layout.vcat(*rows)).numpy()
    sizes = [list(annotation.draw_label(t, "demo/assets/Inter-Regular.otf", 58).shape[1:]) for t in labels]
    rects = rectangles(tile, colors)
    return {"hw": list(hw), "rows": n_rows, "labels": list(labels), "label_sizes": sizes, "height": int(tile.shape[1]),
            "width": int(tile.shape[2]), "panels": [rects[r * n_cols:(r + 1) * n_cols] for r in range(n_rows)]}


def main(root):
    mods = load_reference(root)
    vt = mods["visualization_tools"]
    real_get_cmap = vt.plt.get_cmap
    seen = []

    def recording_get_cmap(name, lut=None):
        cmap = real_get_cmap(name, lut)

        def call(v):
            seen.append(np.array(v, copy=True))
            return cmap(v)
        return call
    vt.plt.get_cmap = recording_get_cmap

    arrays, meta = {}, {"fixtures": {}, "size": [32, 32]}
    e_map = 0.0
    size = (32, 32)
    for name, x in fixtures().items():
        arrays[f"{name}.x"] = x
        h, w, c = x.shape
        basis = given_basis(name, x)
        arrays[f"{name}.basis"] = basis
        xt = torch.from_numpy(x)
        # the range of get_robust_pca for the GIVEN basis
        real_lowrank = torch.pca_lowrank
        torch.pca_lowrank = lambda *_a, **_k: (None, None, torch.from_numpy(basis))
        try:
            _, lo, hi = vt.get_robust_pca(xt.reshape(-1, c))
        finally:
            torch.pca_lowrank = real_lowrank
        arrays[f"{name}.rgb_min"], arrays[f"{name}.rgb_max"] = lo.numpy(), hi.numpy()
        stats = (torch.from_numpy(basis), lo, hi)
        pca = vt.get_pca_map(xt, size, pca_stats=stats)
        arrays[f"{name}.pca_map"] = pca.astype(np.float32)
        seen.clear()
        arrays[f"{name}.scale_rgb"] = vt.get_scale_map(xt[None], size).astype(np.float32)
        arrays[f"{name}.scale_float"] = seen[-1].astype(np.float32)
        seen.clear()
        arrays[f"{name}.sim_rgb"] = vt.get_similarity_map(xt[None].clone(), size).astype(np.float32)
        arrays[f"{name}.sim_float"] = seen[-1].astype(np.float32)
        # the spread of the reference's fp32 evaluation against float64 (same basis and range)
        want = R.resample(R.pca_colors(x, basis, lo.numpy(), hi.numpy()), size, "nearest")
        finite = np.isfinite(want)
        d_pca = float(np.abs(pca - want)[finite].max())
        d_scale = float(np.abs(arrays[f"{name}.scale_float"] - R.resample(R.scale_map(x), size, "nearest")).max())
        d_sim = float(np.abs(arrays[f"{name}.sim_float"] - R.resample(R.similarity_map(x), size, "bilinear")).max())
        meta["fixtures"][name] = {"shape": [h, w, c], "e_pca_map": d_pca, "e_scale": d_scale, "e_sim": d_sim}
        e_map = max(e_map, d_pca, d_scale, d_sim)
    meta["e_map"] = e_map

    # e_pca: torch.pca_lowrank (fp32, q = 3, niter = 20) against float64 eigh, planted-spectrum fixture, 5 seeds
    x = arrays["planted.x"].reshape(-1, 128)
    want, evals = R.pca_basis(x)
    worst = 0.0
    for seed in range(5):
        torch.manual_seed(seed)
        got = torch.pca_lowrank(torch.from_numpy(x), q=3, niter=20)[2].numpy()
        worst = max(worst, float(R.one_minus_abs_cos(got, want).max()))
    meta["e_pca"] = worst
    meta["planted_eigenvalues"] = [float(v) for v in evals]

    meta["offline_tile"] = tile_case(mods, ["Input Image", "Original Feature", "Original Cluster", "Original Norm",
                                            "Original Sim", "Denoised Feat (F)", "Denoised Cluster", "Denoised Norm",
                                            "Denoised Sim", "Shared Noise (G)", "Residual Norm (h)", "Composited (G+h)"], 2,
                                     (40, 56))
    meta["online_tile"] = tile_case(mods, ["Input Image", "Original Feature", "Original Norm", "GT Denoised",
                                           "GT Denoised Norm", "Pred Denoised", "Pred Deno. Norm"], 2, (112, 112))
    meta["get_cluster_map"] = ("not recorded: torch_kmeans is neither installed nor part of the reference's tree; the "
                               "k-means tests use the float64 restatement in tests/vis_reference.py")
    np.savez_compressed(os.path.join(HERE, "vis_reference.npz"), **arrays)
    with open(os.path.join(HERE, "vis_reference.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(json.dumps({k: meta[k] for k in ("e_pca", "e_map")}), os.path.getsize(os.path.join(HERE, "vis_reference.npz")))


if __name__ == "__main__":
    main(sys.argv[1])
