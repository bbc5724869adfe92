"""Time of the visualisation kernels (dvt_amd.vis) per map and per stage-1 tile at 37 x 37 x 768, next to the same maps
computed with torch ops on the same GPU in the reference's way (torch.pca_lowrank + torch.median, a torch Lloyd loop).
Prints one JSON line.

    python tools/bench_vis.py [--reps 20] [--rows 6]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "denoising-vit_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from dvt_amd import vis as VS  # noqa: E402
from dvt_amd.utils import visualization as VZ  # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def torch_robust_pca(x, m=2.0):
    basis = torch.pca_lowrank(x, q=3, niter=20)[2]
    colors = x @ basis
    d = (colors - colors.median(dim=0).values).abs()
    s = d / d.median(dim=0).values
    lo = torch.stack([colors[s[:, c] < m, c].min() for c in range(3)])
    hi = torch.stack([colors[s[:, c] < m, c].max() for c in range(3)])
    return ((colors - lo) / (hi - lo)).clamp(0, 1)


def torch_kmeans(x, starts, max_iter=100, tol=1e-4):
    xn = torch.nn.functional.normalize(x, dim=1)
    best = None
    for rows in starts:
        cen = x[rows]
        for _ in range(max_iter):
            lab = (xn @ torch.nn.functional.normalize(cen, dim=1).T).argmax(1)
            one = torch.nn.functional.one_hot(lab, cen.shape[0]).to(x.dtype)
            cnt = one.sum(0)
            new = torch.where(cnt[:, None] > 0, (one.T @ x) / cnt.clamp(min=1)[:, None], cen)
            shift = ((new - cen) ** 2).sum()
            cen = new
            if float(shift) < tol:  # the host round trip per iteration of a library loop
                break
        inertia = float((1 - (xn * torch.nn.functional.normalize(cen, dim=1)[lab]).sum(1)).sum())
        if best is None or inertia < best[0]:
            best = (inertia, lab)
    return best[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=6, help="rows of the stage-1 tile (num_vis_samples + 1)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h = w = 37
    c, k = 768, 5
    rng = np.random.RandomState(0)
    dirs = rng.standard_normal((k, c))
    lab = rng.randint(0, k, h * w)
    x = torch.from_numpy((1.0 * dirs[lab] + rng.standard_normal((h * w, c))).astype(np.float32)).to(dev).reshape(h, w, c)
    eng = VS.VisEngine(dev, max_rows=h * w, max_channels=c, max_clusters=k)
    starts = VS.kmeans_start_rows(h * w, k, VS.KMEANS_NUM_INIT, np.random.RandomState(0))
    starts_t = torch.from_numpy(starts).to(dev).long()
    eng.new_canvas(518, 518)
    rect = (0, 0, 518, 518)
    out = {"shape": [h, w, c], "reps": a.reps}
    out["hip_ms"] = {
        "pca_map": timed(lambda: eng.pca_map(x), a.reps),
        "cluster_map": timed(lambda: eng.kmeans(x, k, init_rows=starts), a.reps),
        "scale_map": timed(lambda: eng.scale_map(x), a.reps),
        "similarity_map": timed(lambda: eng.similarity_map(x), a.reps),
        "render_518": timed(lambda: eng.render_scalar(x[..., 0], rect, "turbo", "bilinear", neg_red=True), a.reps),
    }
    km = eng.kmeans(x, k, init_rows=starts)
    out["kmeans_iterations"] = km["iterations"].cpu().tolist()
    flat = x.reshape(-1, c)
    out["torch_ms"] = {
        "pca_map": timed(lambda: torch_robust_pca(flat), a.reps),
        "cluster_map": timed(lambda: torch_kmeans(flat, starts_t), max(2, a.reps // 5), warmup=1),
        "scale_map": timed(lambda: (lambda n: (n - n.min()) / (n.max() - n.min() + 1e-6))(flat.norm(dim=1)), a.reps),
        "similarity_map": timed(lambda: torch.nn.functional.normalize(flat, dim=1) @ torch.nn.functional.normalize(flat[684], dim=0), a.reps),
    }
    # one stage-1 tile: `rows` rows of 12 panels at 518 x 518 (5 PCA maps, 2 cluster maps, 3 norm maps, 2 similarity maps each)
    images = torch.rand(a.rows, 3, 518, 518, device=dev)

    def tile():
        t = VZ._Tile(eng, a.rows, 12, (518, 518), VZ.OFFLINE_LABELS, None)
        r = np.random.RandomState(0)
        for i in range(a.rows):
            eng.render_rgb(images[i], t.rect(i, 0), planar=True)
            VZ._feature_panels(eng, t, i, 1, x, r)
            VZ._feature_panels(eng, t, i, 5, x, r)
            eng.render_rgb(eng.pca_map(x)[0], t.rect(i, 9))
            eng.render_scalar(eng.scale_map(x), t.rect(i, 10), "inferno")
            eng.render_rgb(eng.pca_map(x)[0], t.rect(i, 11))
        return eng.canvas_u8()
    out["tile_ms"] = timed(tile, max(2, a.reps // 5), warmup=1)
    pca_launches = (2 + VS.PCA_ITERS + 1) + 1 + 2 + 1  # basis, projection, range, colours
    km_launches = 3 * VS.KMEANS_MAX_ITER + 4
    per_row = 5 * (pca_launches + 1) + 2 * (km_launches + 1) + 3 * 3 + 2 * 3 + 1
    out["launches_per_tile_formula"] = a.rows * per_row + 12 + 2  # from the launch counts of include/dvt_vis.h, not counted
    out["launches_per_tile_note"] = f"{km_launches} per cluster map, most of them no-ops once a restart has converged"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
