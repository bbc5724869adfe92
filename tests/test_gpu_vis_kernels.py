"""GPU: the visualisation kernels (csrc/dvt_vis.hip) against the float64 reference in tests/vis_reference.py, on the
committed fixtures and on seeded maps at the real shapes.

Tolerances: e_pca / e_map are the reference-vs-float64 spreads MEASURED by tests/golden/make_vis_golden.py and read from
tests/golden/vis_reference.json; the bounds are max(4 * e, 1e-6).  The k-means margin C * 2^-22 bounds the fp32 error of the
difference of two C-term dot products of unit vectors (the kernel accumulates them in fp64, which is stricter).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import vis_reference as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("planted", "odd", "zero_dev", "duplicates")
REAL_SHAPES = ((37, 37, 768), (37, 37, 1024), (16, 16, 384))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "vis_reference.npz")), json.load(open(os.path.join(GOLDEN, "vis_reference.json")))


@pytest.fixture(scope="module")
def eng(built_lib):
    from dvt_amd.vis import VisEngine
    return VisEngine(DEV, max_rows=8 * 37 * 37, max_channels=1024, max_clusters=16, max_init=8)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype)


def seeded_map(shape, seed):
    """A map with structure: a few smooth components with a decaying spectrum over noise."""
    h, w, c = shape
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    comps = np.stack([np.sin(3 * xx + yy), np.cos(2 * yy - xx), xx * yy, np.sin(5 * yy)], -1)
    x = comps @ (rng.standard_normal((4, c)) * np.array([6.0, 3.5, 2.0, 1.2])[:, None]) + 0.3 * rng.standard_normal((h, w, c))
    return (x + rng.standard_normal(c)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- PCA
def test_pca_basis_on_the_planted_fixture(eng, gold):
    arrays, meta = gold
    x = arrays["planted.x"]
    bound = max(4 * meta["e_pca"], 1e-6)
    basis, evals = eng.pca_basis(dev(x))
    want, wev = R.pca_basis(x)
    err = R.one_minus_abs_cos(basis.cpu().numpy(), want)
    print("pca planted 1-|cos|", err, "bound", bound, "evals", evals.cpu().numpy(), wev)
    assert (err <= bound).all()
    b = basis.cpu().numpy()
    assert np.allclose(np.linalg.norm(b, axis=0), 1.0, atol=1e-5)
    for j in range(3):  # the sign rule, exactly: the largest-magnitude component (lowest index) is positive
        assert b[np.argmax(np.abs(b[:, j])), j] > 0
        assert np.sign(b[:, j] @ want[:, j]) > 0
    assert np.allclose(evals.cpu().numpy(), wev, rtol=1e-4)
    # same input twice, and with a NaN-filled workspace: identical bits
    again, ev2 = eng.pca_basis(dev(x))
    eng.work.view(torch.float32).fill_(float("nan"))
    third, ev3 = eng.pca_basis(dev(x))
    assert torch.equal(basis, again) and torch.equal(basis, third) and torch.equal(evals, ev2) and torch.equal(evals, ev3)


@pytest.mark.parametrize("shape", REAL_SHAPES)
def test_pca_basis_at_the_real_shapes(eng, shape):
    """Seeded maps with separated leading directions (ratios of the leading eigenvalues printed); masked subset too."""
    x = seeded_map(shape, 5)
    want, wev = R.pca_basis(x)
    basis, _ = eng.pca_basis(dev(x))
    err = R.one_minus_abs_cos(basis.cpu().numpy(), want)
    print("pca", shape, "1-|cos|", err, "eigenvalues", wev)
    assert (err <= 1e-6).all()
    mask = np.random.RandomState(1).rand(shape[0] * shape[1]) < 0.6
    wantm, _ = R.pca_basis(x, mask)
    bm, _ = eng.pca_basis(dev(x), dev(mask.astype(np.uint8), torch.uint8))
    assert (R.one_minus_abs_cos(bm.cpu().numpy(), wantm) <= 1e-6).all()


# ---------------------------------------------------------------------------------------------------------------- range
def check_range(eng, colors32, mask=None):
    lo, hi, det = eng.robust_range(dev(colors32), None if mask is None else dev(mask, torch.uint8), 2.0, details=True)
    want = R.robust_range(colors32.astype(np.float64), mask, 2.0)
    rows = det["rows"].cpu().numpy()
    assert np.array_equal(rows, want["rows"]), (rows, want["rows"])
    assert np.array_equal(det["median"].cpu().numpy(), want["median"])
    assert np.array_equal(det["deviation"].cpu().numpy(), want["deviation"])
    assert np.array_equal(lo.cpu().numpy(), want["rgb_min"].astype(np.float32))
    assert np.array_equal(hi.cpu().numpy(), want["rgb_max"].astype(np.float32))
    return want


@pytest.mark.parametrize("name", FIXTURES)
def test_robust_range_selects_the_references_rows(eng, gold, name):
    """The basis is GIVEN and the projected rows are handed to both sides, so the selection is tested alone: the median,
    deviation, minimum and maximum are the same ROWS (even / odd counts, duplicates, the zero-deviation fall-back)."""
    arrays, _ = gold
    x, basis = arrays[f"{name}.x"], arrays[f"{name}.basis"]
    colors = eng.project(dev(x), dev(basis)).cpu().numpy()
    assert np.abs(colors - x.reshape(-1, x.shape[-1]).astype(np.float64) @ basis.astype(np.float64)).max() < 1e-4
    want = check_range(eng, colors)
    assert want["rows"][12] == (1 if name == "zero_dev" else 0)
    # and what the reference itself recorded for this basis
    lo, hi = eng.robust_range(dev(colors))
    assert np.allclose(lo.cpu().numpy(), arrays[f"{name}.rgb_min"], atol=1e-5)
    assert np.allclose(hi.cpu().numpy(), arrays[f"{name}.rgb_max"], atol=1e-5)


def test_robust_range_large_masked_and_duplicated(eng):
    rng = np.random.RandomState(3)
    for n in (8 * 1369, 1369, 1368, 2, 1):
        colors = (rng.standard_normal((n, 3)) * [1.0, 10.0, 1e-3] + [0.0, -5.0, 2.0]).astype(np.float32)
        check_range(eng, colors)
        colors[rng.randint(0, n, n // 2)] = colors[0]  # many exact duplicates
        check_range(eng, colors)
        if n > 4:
            check_range(eng, colors, (rng.rand(n) < 0.5).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------------- maps
def map_bound(meta):
    return max(4 * meta["e_map"], 1e-6)


@pytest.mark.parametrize("name", FIXTURES)
def test_maps_on_the_fixtures(eng, gold, name):
    arrays, meta = gold
    x = arrays[f"{name}.x"]
    bound = map_bound(meta)
    stats = (arrays[f"{name}.basis"], arrays[f"{name}.rgb_min"], arrays[f"{name}.rgb_max"])
    got, _ = eng.pca_map(dev(x), tuple(dev(s) for s in stats))
    want = R.pca_colors(x, *stats)
    finite = np.isfinite(want)
    errs = [np.abs(got.cpu().numpy() - want)[finite].max(),
            np.abs(eng.scale_map(dev(x)).cpu().numpy() - R.scale_map(x)).max(),
            np.abs(eng.similarity_map(dev(x)).cpu().numpy() - R.similarity_map(x)).max()]
    print("maps", name, errs, "bound", bound)
    assert max(errs) <= bound


@pytest.mark.parametrize("shape", REAL_SHAPES)
def test_maps_at_the_real_shapes(eng, gold, shape):
    bound = map_bound(gold[1])
    x = seeded_map(shape, 9)
    basis, lo, hi = R.robust_pca(x)
    got, _ = eng.pca_map(dev(x), (dev(basis), dev(lo), dev(hi)))
    errs = [np.abs(got.cpu().numpy() - R.pca_colors(x, basis.astype(np.float32), lo.astype(np.float32), hi.astype(np.float32))).max(),
            np.abs(eng.scale_map(dev(x)).cpu().numpy() - R.scale_map(x)).max(),
            np.abs(eng.similarity_map(dev(x)).cpu().numpy() - R.similarity_map(x)).max()]
    print("maps", shape, errs, "bound", bound)
    assert max(errs) <= bound
    sim = eng.similarity_map(dev(x)).cpu().numpy()
    assert sim[shape[0] // 2, shape[1] // 2] == -1.0
    # fitted on the device end to end: the colours of the device's own basis and range
    colors, (b, l, h) = eng.pca_map(dev(x))
    want = R.pca_colors(x, b.cpu().numpy(), l.cpu().numpy(), h.cpu().numpy())
    assert np.abs(colors.cpu().numpy() - want).max() <= bound
    again, _ = eng.pca_map(dev(x))
    assert torch.equal(colors, again)


# ---------------------------------------------------------------------------------------------------------------- k-means
def test_kmeans_lock_step(eng):
    """One assignment + update (max_iter = 1) from GIVEN centres, fed from the float64 trajectory step after step."""
    n, c, k = 1369, 768, 5
    rng = np.random.RandomState(21)
    dirs = rng.standard_normal((k, c))
    lab = rng.randint(0, k, n)
    x = (0.3 * dirs[lab] + rng.standard_normal((n, c))).astype(np.float32)  # rows = scale * direction[label] + N(0, 1)
    margin = c * 2.0 ** -22
    xd = dev(x)
    worst_excluded, steps = 0.0, 0
    for start in range(8):
        cen = x[rng.choice(n, k, replace=False)].astype(np.float64)
        for _ in range(100):
            ref = R.kmeans_step(x, cen)
            sure = ref["margin"] > margin
            excluded = 1.0 - sure.mean()
            worst_excluded = max(worst_excluded, excluded)
            assert excluded <= 0.02, f"the input breaks the test's condition: {excluded:.4f} of the rows within the margin"
            out = eng.kmeans(xd, k, init_centers=cen.astype(np.float32)[None], max_iter=1, tol=0.0)
            got_lab = out["labels"].cpu().numpy()
            assert np.array_equal(got_lab[sure], ref["labels"][sure])
            # the kernel started from the fp32 image of the centres; its update against float64 means of ITS labels
            want_cen = R.kmeans_step(x, cen.astype(np.float32), labels=got_lab)["centers"]
            got_cen = out["centers"].cpu().numpy()
            rel = np.abs(got_cen - want_cen).max(axis=1) / np.abs(want_cen).max(axis=1)
            assert rel.max() <= 1e-5, rel
            assert int(out["iterations"][0]) == 1
            assert abs(float(out["inertia"][0]) - R.kmeans_step(x, cen.astype(np.float32))["inertia"]) <= 1e-6 * n
            steps += 1
            cen = ref["centers"]
            if ref["shift"] < 1e-4:
                break
    print("kmeans lock-step:", steps, "steps, worst excluded share", worst_excluded)


def test_kmeans_full_run(eng):
    """A well-separated mixture, one start row from each planted component: every restart ends in the planted partition,
    so the 8 inertias agree to rounding and say nothing about the choice of the restart -- that is
    test_kmeans_restart_selection's subject."""
    n, c, k = 1369, 768, 5
    rng = np.random.RandomState(4)
    dirs = rng.standard_normal((k, c))
    planted = rng.randint(0, k, n)
    x = (2.0 * dirs[planted] + rng.standard_normal((n, c))).astype(np.float32)
    starts = np.stack([[rng.choice(np.nonzero(planted == j)[0]) for j in rng.permutation(k)] for _ in range(8)]).astype(np.int32)
    ref = R.kmeans(x, x[starts].astype(np.float64))
    out = eng.kmeans(dev(x), k, init_rows=starts)
    assert np.array_equal(out["iterations"].cpu().numpy(), ref["iterations"]) and (ref["iterations"] <= 3).all()
    inertia = out["inertia"].cpu().numpy()
    assert np.allclose(inertia, ref["inertia"], rtol=1e-9)
    best = int(out["best"][0])
    assert inertia[best] == inertia.min() and (inertia[:best] > inertia[best]).all()  # lowest index among equal ones
    one = R.kmeans(x, x[starts[best:best + 1]].astype(np.float64))
    got = out["labels"].cpu().numpy()
    assert np.array_equal(got, one["labels"])
    assert len({(a, b) for a, b in zip(got, planted)}) == k  # the planted partition, up to the naming of the clusters
    assert np.abs(out["centers"].cpu().numpy() - one["centers"]).max() < 1e-4


def test_kmeans_restart_selection(eng):
    """Restarts whose inertias really differ: labels, iteration counts, the ORDER of the per-restart inertias and the winning
    restart equal the float64 reference's.

    Six planted components, two pairs of them correlated (0.6 and 0.4), five clusters; each start takes one row from five
    components and leaves out one member of a correlated pair, whose rows then join their partner (similarity about 0.5
    against 0 for the others: no row within the margin C * 2^-22 in any step, asserted).  Leaving out a member of the first
    pair ends in one local optimum, of the second pair in another; only restart 3 reaches the better one, so the winner is
    defined.  Inside the worse optimum the seven inertias agree to rounding, so the order is compared between the optima
    here, and completely with max_iter = 1, where every restart's inertia is that of its own start rows and all differ."""
    n, c, k = 1369, 768, 5
    rng = np.random.RandomState(4)
    d = rng.standard_normal((6, c))
    d /= np.linalg.norm(d, axis=1, keepdims=True)

    def mix(a, b, r):
        o = b - (b @ a) * a
        return r * a + np.sqrt(1 - r * r) * o / np.linalg.norm(o)
    d[1], d[3] = mix(d[0], d[1], 0.6), mix(d[2], d[3], 0.4)
    planted = rng.randint(0, 6, n)
    x = (2.0 * np.sqrt(c) * d[planted] + rng.standard_normal((n, c))).astype(np.float32)
    starts = []
    for omit in (2, 3, 2, 0, 3, 2, 3, 2):
        comps = [j for j in range(6) if j != omit]
        starts.append([rng.choice(np.nonzero(planted == comps[i])[0]) for i in rng.permutation(5)])
    starts = np.array(starts, np.int32)
    margin = c * 2.0 ** -22
    for row in starts:  # the condition on the input, on the reference's own trajectory
        cen = x[row].astype(np.float64)
        for _ in range(100):
            st = R.kmeans_step(x, cen)
            assert st["margin"].min() > margin
            cen = st["centers"]
            if st["shift"] < 1e-4:
                break
    xd = dev(x)
    ref = R.kmeans(x, x[starts].astype(np.float64))
    out = eng.kmeans(xd, k, init_rows=starts)
    inertia = out["inertia"].cpu().numpy()
    print("kmeans restarts: inertia", inertia, "reference", ref["inertia"], "best", int(out["best"][0]), ref["best"])
    assert ref["best"] == 3 and np.sort(ref["inertia"])[1] - ref["inertia"][3] > 1.0  # two optima, one winner
    assert int(out["best"][0]) == ref["best"]
    assert np.array_equal(out["iterations"].cpu().numpy(), ref["iterations"])
    assert np.allclose(inertia, ref["inertia"], rtol=1e-9)
    assert np.array_equal(inertia < inertia.mean(), ref["inertia"] < ref["inertia"].mean())
    assert np.array_equal(out["labels"].cpu().numpy(), ref["labels"])
    assert np.abs(out["centers"].cpu().numpy() - ref["centers"]).max() < 1e-4
    # max_iter = 1: eight distinct inertias, the complete order and the winner
    ref1 = R.kmeans(x, x[starts].astype(np.float64), max_iter=1, tol=0.0)
    gaps = np.diff(np.sort(ref1["inertia"]))
    assert gaps.min() > 1e-6 * ref1["inertia"].max()
    out1 = eng.kmeans(xd, k, init_rows=starts, max_iter=1, tol=0.0)
    in1 = out1["inertia"].cpu().numpy()
    assert np.array_equal(np.argsort(in1, kind="stable"), np.argsort(ref1["inertia"], kind="stable"))
    assert int(out1["best"][0]) == ref1["best"]
    assert np.array_equal(out1["iterations"].cpu().numpy(), ref1["iterations"])
    assert np.array_equal(out1["labels"].cpu().numpy(), ref1["labels"])
    # a restart from all-zero centres: similarity 0 everywhere (no NaN), inertia n exactly, and it loses
    cen = np.concatenate([np.zeros((1, k, c), np.float32), x[starts[3:4]]])
    outz = eng.kmeans(xd, k, init_centers=cen, max_iter=1, tol=0.0)
    assert int(outz["best"][0]) == 1 and float(outz["inertia"][0]) == float(n)


def test_kmeans_ties_limits_and_empty_clusters(eng):
    n, c, k = 1369, 768, 5
    rng = np.random.RandomState(8)
    dirs = rng.standard_normal((k, c))
    planted = rng.randint(0, k, n)
    x = (2.0 * dirs[planted] + rng.standard_normal((n, c))).astype(np.float32)
    xd = dev(x)
    # two start rows from one component: only what does not depend on ties
    rows0 = np.nonzero(planted == 0)[0][:2]
    start = np.concatenate([rows0, [np.nonzero(planted == j)[0][0] for j in (1, 2, 3)]]).astype(np.int32)[None]
    a = eng.kmeans(xd, k, init_rows=start, max_iter=100)
    eng.work.view(torch.float32).fill_(float("nan"))
    b = eng.kmeans(xd, k, init_rows=start, max_iter=100)
    for key in a:
        assert torch.equal(a[key], b[key]), key
    assert 1 <= int(a["iterations"][0]) <= 100
    lab = a["labels"].cpu().numpy()
    assert lab.min() >= 0 and lab.max() < k
    # max_iter reached is reported, not an error
    short = eng.kmeans(xd, k, init_rows=start, max_iter=1, tol=0.0)
    assert int(short["iterations"][0]) == 1
    # a centre no row prefers stays where it was
    far = -x.mean(axis=0, keepdims=True)
    cen = np.concatenate([x[[np.nonzero(planted == j)[0][0] for j in range(4)]], far]).astype(np.float32)
    ref = R.kmeans_step(x, cen)
    assert not (ref["labels"] == 4).any()
    out = eng.kmeans(xd, k, init_centers=cen[None], max_iter=1, tol=0.0)
    assert np.array_equal(out["centers"].cpu().numpy()[4], cen[4])
    assert np.array_equal(out["labels"].cpu().numpy(), ref["labels"])
    # identical rows: every similarity ties, the lowest cluster wins
    same = np.tile(x[:1], (64, 1))
    out = eng.kmeans(dev(same), 3, init_centers=np.tile(x[:1], (3, 1))[None], max_iter=2)
    assert (out["labels"].cpu().numpy() == 0).all()


# ---------------------------------------------------------------------------------------------------------------- render
@pytest.mark.parametrize("interp", ["nearest", "bilinear"])
@pytest.mark.parametrize("src,dst", [((37, 37), (518, 518)), ((16, 16), (224, 224)), ((5, 7), (33, 20)), ((12, 12), (12, 12)),
                                     ((37, 37), (20, 31))])
def test_resampling_matches_torch(eng, interp, src, dst):
    rng = np.random.RandomState(2)
    smap = rng.rand(*src).astype(np.float32)
    rgb = rng.rand(*src, 3).astype(np.float32)
    kw = {"align_corners": False} if interp == "bilinear" else {}
    eng.new_canvas(dst[0] + 5, dst[1] + 9, (0.5, 0.25, 0.125))
    rect = (2, 4, dst[0], dst[1])
    eng.render_scalar(dev(smap), rect, None, interp)
    got = eng.canvas.cpu().numpy()
    want = torch.nn.functional.interpolate(torch.from_numpy(smap)[None, None], size=dst, mode=interp, **kw)[0, 0].numpy()
    assert np.abs(got[:, 2:2 + dst[0], 4:4 + dst[1]] - want[None]).max() <= 1e-6
    outside = np.ones(got.shape[1:], bool)
    outside[2:2 + dst[0], 4:4 + dst[1]] = False
    assert (got[0][outside] == 0.5).all() and (got[1][outside] == 0.25).all() and (got[2][outside] == 0.125).all()
    for planar in (False, True):
        eng.render_rgb(dev(rgb.transpose(2, 0, 1) if planar else rgb), rect, interp, planar=planar)
        got = eng.canvas.cpu().numpy()[:, 2:2 + dst[0], 4:4 + dst[1]]
        want = torch.nn.functional.interpolate(torch.from_numpy(rgb).permute(2, 0, 1)[None], size=dst, mode=interp, **kw)[0].numpy()
        assert np.abs(got - want).max() <= 1e-6


def test_table_lookup_labels_red_rule_and_u8(eng):
    table = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7) % 256], 1).astype(np.float32) / 255
    v = np.concatenate([[-0.5, 1.5, 0.5, 1 / 256, 255 / 256, np.nextafter(np.float32(1 / 256), np.float32(0))],
                        np.linspace(0, 1, 63 * 63 - 6)]).astype(np.float32).reshape(63, 63)
    eng.new_canvas(63, 63)
    eng.render_scalar(dev(v), (0, 0, 63, 63), dev(table))
    got = eng.canvas.permute(1, 2, 0).cpu().numpy()
    assert np.array_equal(got, R.apply_table(v, table).astype(np.float32))
    eng.render_scalar(dev(v - 0.25), (0, 0, 63, 63), dev(table), neg_red=True)
    got = eng.canvas.permute(1, 2, 0).cpu().numpy()
    want = R.apply_table(v - np.float32(0.25), table).astype(np.float32)
    want[(v - np.float32(0.25)) < 0] = (1, 0, 0)
    assert np.array_equal(got, want)
    assert np.array_equal(eng.canvas_u8().cpu().numpy(), R.to_u8(want))
    labels = np.random.RandomState(0).randint(0, 5, (9, 11)).astype(np.int32)
    eng.new_canvas(45, 44)
    eng.render_labels(dev(labels, torch.int32), (0, 0, 45, 44), 5)
    from dvt_amd.vis import color_table
    got = eng.canvas.permute(1, 2, 0).cpu().numpy()
    assert np.array_equal(got, R.labels_panel(labels, (45, 44), color_table("rainbow", 5)).astype(np.float32))


def test_rectangles_outside_the_canvas_are_rejected(eng):
    from dvt_amd import _lib
    eng.new_canvas(16, 16)
    for rect in ((-1, 0, 4, 4), (0, 0, 0, 4), (13, 0, 4, 4), (0, 14, 4, 3), (0, 0, 17, 16)):
        with pytest.raises(_lib.DvtError):
            eng.render_scalar(torch.zeros(2, 2, device=DEV), rect)
        with pytest.raises(_lib.DvtError):
            eng.fill(rect)
    with pytest.raises(_lib.DvtError):
        eng.scale_map(torch.zeros(4, 4, 64))  # a CPU tensor: no fallback
