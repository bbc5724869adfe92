"""GPU: the video-demo kernels (csrc/dvt_video.hip) against the float64 restatement in tests/video_reference.py, on seeded
maps at 120 x 211 x 768, 37 x 37 x 1024 and a tiny odd one (5 x 7 x 64).

Bounds: P and the norms within max(4 e_map, 1e-6) relative to the column scale, e_map read from
tests/golden/vis_reference.json as tests/test_gpu_vis_kernels.py does; the softmax-of-norm map within the same bound
(absolute: the map lies in [0, 1]); labels equal to the float64 labels at every row whose two largest cosines differ by more
than C 2^-22 (the margin rule of the k-means tests); masks equal at every row whose float64 value is farther from the
threshold than the bound.  The uint8 stages are exact given the same inputs: numpy's float32 arithmetic on the kernel's own
P / range / labels, and PIL's resize of the kernel's own token pictures.

The maps are at the scale of final-normed ViT tokens (row norms of a few tens): the script's softmax(|x| / 5) presumes that
scale, and a fp32 norm carries a relative error of 2^-24 that the exponential turns into |x| / 5 x 2^-24 relative.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import video_reference as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
SHAPES = (((120, 211, 768), (490, 854)), ((37, 37, 1024), (518, 518)), ((5, 7, 64), (33, 20)))
K = 8


def bound():
    return max(4 * json.load(open(os.path.join(GOLDEN, "vis_reference.json")))["e_map"], 1e-6)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype)


def make_case(shape, out_hw, seed=11):
    from dvt_amd import video as VD
    gh, gw, c = shape
    rng = np.random.RandomState(seed)
    x = R.seeded_feature_map(shape, seed)
    M = (rng.standard_normal((c, VD.N_COLS)) / np.sqrt(c)).astype(np.float32)
    centers = (x.reshape(-1, c)[rng.choice(gh * gw, K, replace=False)] + 0.1 * rng.standard_normal((K, c))).astype(np.float32)
    stats = {"reduct_mat_full": M[:, 3:6].copy(), "standard_mapping": M[:, 6:7].copy()}
    eng = VD.VideoDemoEngine(DEV, (gh, gw), c, out_hw, stats, num_clusters=K, seed=0)
    eng.M, eng.centers = dev(M), dev(centers)
    return eng, x.reshape(-1, c), M, centers


def snapshot(pics, det):
    out = {f"full.{k}": v.clone() for k, v in pics.items()}
    out.update({f"token.{k}": v.clone() for k, v in det["token"].items()})
    out.update({k: det[k].clone() for k in det if k != "token"})
    return out


@pytest.mark.parametrize("shape,out_hw", SHAPES)
def test_frame_kernels_against_float64(built_lib, shape, out_hw):
    from dvt_amd import video as VD
    eng, x, M, centers = make_case(shape, out_hw)
    gh, gw, c = shape
    n, b = gh * gw, bound()
    xd = dev(x)
    first = snapshot(*eng.frame(xd, details=True))
    # ---- same input again, every output buffer filled with NaN / 0xff first: identical bits
    for t in (eng.P, eng.norms, eng.norm_map, eng.range, eng.range_second):
        t.fill_(float("nan"))
    for t in (eng.labels, eng.mask_fg, eng.mask_standard, eng.token, eng.tmp, eng.full):
        t.fill_(-1 if t.dtype == torch.int32 else 255)
    eng.vis.work.view(torch.float32).fill_(float("nan"))
    second = snapshot(*eng.frame(xd, details=True))
    for k in first:
        assert torch.equal(first[k], second[k]), k
    g = {k: v.cpu().numpy() for k, v in first.items()}
    # ---- apply: P, norms, labels
    v = R.frame_values(x, M[:, 0:3], M[:, 3:6], M[:, 6:7], M[:, 7:10], M[:, 10:13], centers)
    P64 = x.astype(np.float64) @ M.astype(np.float64)
    err_p = (np.abs(g["P"] - P64) / np.abs(P64).max(0, keepdims=True)).max()
    err_n = np.abs(g["norms"] - v["norms"]).max() / v["norms"].max()
    err_s = np.abs(g["norm_map"] - v["norm_map"]).max()
    print(f"{shape}: P {err_p:.2e} norms {err_n:.2e} softmax-norm map {err_s:.2e} (bound {b:.2e}); row norms "
          f"{v['norms'].min():.1f} .. {v['norms'].max():.1f}")
    assert err_p <= b and err_n <= b and err_s <= b
    sure = v["label_gap"] > c * 2.0 ** -22
    print(f"{shape}: {int((~sure).sum())} of {n} rows within the k-means margin; clusters used {np.unique(v['labels']).size}")
    assert np.array_equal(g["labels"][sure], v["labels"][sure])
    assert sure.mean() > 0.9
    # ---- col_range: the minimum / maximum of the kernel's own P, exactly
    P = g["P"]
    assert np.array_equal(g["range"], np.stack([P.min(0), P.max(0)]))
    second_col = np.float32(-1.0) * P[:, VD.COL_DATASET + 1] + np.float32(1.0)
    assert np.array_equal(g["range_second"], np.array([second_col.min(), second_col.max()], np.float32))
    # ---- masks
    colscale = np.abs(P64).max(0)
    sure_fg = np.abs(v["second"] - 0.1) > b * colscale[VD.COL_DATASET + 1]
    sure_std = np.abs(v["standard"]) > b * colscale[VD.COL_STANDARD]
    print(f"{shape}: rows within the bound of a mask threshold: {int((~sure_fg).sum())} / {int((~sure_std).sum())}; foreground "
          f"{v['mask_fg'].mean():.3f} / {v['mask_standard'].mean():.3f}")
    assert np.array_equal(g["mask_fg"][sure_fg].astype(bool), v["mask_fg"][sure_fg])
    assert np.array_equal(g["mask_standard"][sure_std].astype(bool), v["mask_standard"][sure_std])
    assert np.array_equal(g["mask_fg"].astype(bool), second_col > np.float32(0.1))  # and exactly, in fp32, on its own P
    assert np.array_equal(g["mask_standard"].astype(bool), P[:, VD.COL_STANDARD] > 0)
    assert 0 < g["mask_fg"].sum() < n or n < 100
    # ---- token pictures: numpy's float32 arithmetic on the kernel's own P / range / labels / masks
    lo, hi = g["range"]
    unit = (P - lo[None]) / (hi - lo)[None]
    assert unit.dtype == np.float32

    def u8(a):
        return (a * np.float32(255)).astype(np.uint8)
    inferno, rainbow = VD.color_table_u8("inferno"), VD.label_table_u8("rainbow", K)

    def through(vals):
        return inferno[np.minimum((vals * np.float32(256)).astype(np.int64), 255)]
    second_unit = (second_col - g["range_second"][0]) / (g["range_second"][1] - g["range_second"][0])
    want = {"pca_instance": u8(unit[:, 0:3]), "pca_dataset": u8(unit[:, 3:6]),
            "fg_pca": u8(unit[:, 7:10] * g["mask_fg"][:, None].astype(np.float32)),
            "fg_pca_standard": u8(unit[:, 10:13] * g["mask_standard"][:, None].astype(np.float32)),
            "first_pca": through(unit[:, 3]), "second_pca": through(second_unit), "third_pca": through(unit[:, 5]),
            "norm": through(g["norm_map"]), "kmeans": rainbow[g["labels"]]}
    for kind in R.MAP_KINDS:
        tok = g[f"token.{kind}"]
        assert np.array_equal(tok.reshape(-1, 3), want[kind]), kind
        pil = np.asarray(Image.fromarray(tok).resize((out_hw[1], out_hw[0]), Image.BICUBIC))
        assert np.array_equal(g[f"full.{kind}"], pil), kind
    assert len({g[f"token.{k}"].tobytes() for k in R.MAP_KINDS}) == len(R.MAP_KINDS)  # nine different pictures


@pytest.mark.parametrize("shape,out_hw", SHAPES[:2])
def test_resize_is_pillows(built_lib, shape, out_hw):
    """The random / constant / checkerboard images of the CPU test through the device's resize, three at a time."""
    from tests.test_video_cpu import pil_resize, resize_inputs
    eng, _, _, _ = make_case(shape, out_hw)
    imgs = resize_inputs(shape[:2])
    src = dev(np.stack(list(imgs.values())), torch.uint8)
    dst = torch.full((len(imgs), out_hw[0], out_hw[1], 3), 7, dtype=torch.uint8, device=DEV)
    tmp = torch.empty((len(imgs), shape[0], out_hw[1], 3), dtype=torch.uint8, device=DEV)
    eng.resize(src, dst, tmp)
    got = dst.cpu().numpy()
    for i, (name, a) in enumerate(imgs.items()):
        assert np.array_equal(got[i], pil_resize(a, out_hw)), name


def test_bad_arguments_write_nothing(built_lib):
    from dvt_amd import _lib
    L = _lib.lib()
    n, c, m = 64, 64, 4
    x, M, cen = torch.randn(n, c, device=DEV), torch.randn(c, 33, device=DEV), torch.randn(17, c, device=DEV)
    P = torch.full((n, 33), 5.0, device=DEV)
    norms = torch.full((n,), 5.0, device=DEV)
    labels = torch.full((n,), 5, dtype=torch.int32, device=DEV)
    rng = torch.full((2, 33), 5.0, device=DEV)
    u8 = torch.full((n, 3), 5, dtype=torch.uint8, device=DEV)
    table = torch.zeros((256, 3), dtype=torch.uint8, device=DEV)
    i32 = torch.zeros((64, 5), dtype=torch.int32, device=DEV)
    s = _lib.stream()
    p = lambda t: t.data_ptr()  # noqa: E731
    bad = [
        L.dvt_video_apply(p(x), n, c, p(M), 33, None, 0, p(P), p(norms), None, s),              # m > 32
        L.dvt_video_apply(p(x), n, c, p(M), m, p(cen), 17, p(P), p(norms), p(labels), s),       # K > DVT_VIS_MAX_K
        L.dvt_video_apply(p(x), 0, c, p(M), m, None, 0, p(P), p(norms), None, s),               # n = 0
        L.dvt_video_apply(None, n, c, p(M), m, None, 0, p(P), p(norms), None, s),
        L.dvt_video_apply(p(x), n, c, None, m, None, 0, p(P), p(norms), None, s),
        L.dvt_video_apply(p(x), n, c, p(M), m, None, 0, None, p(norms), None, s),
        L.dvt_video_apply(p(x), n, c, p(M), m, p(cen), 8, p(P), p(norms), None, s),             # centres without labels
        L.dvt_video_apply(p(x), n, 96, p(M), m, None, 0, p(P), p(norms), None, s),              # C % 64
        L.dvt_video_col_range(p(P), n, 33, p(rng), -1, 1.0, 0.0, None, s),
        L.dvt_video_col_range(p(P), 0, m, p(rng), -1, 1.0, 0.0, None, s),
        L.dvt_video_col_range(None, n, m, p(rng), -1, 1.0, 0.0, None, s),
        L.dvt_video_col_range(p(P), n, m, p(rng), 1, 1.0, 0.0, None, s),                        # affine column without its output
        L.dvt_video_softmax_norm_map(p(norms), 0, 5.0, p(P), s),
        L.dvt_video_softmax_norm_map(None, n, 5.0, p(P), s),
        L.dvt_video_softmax_norm_map(p(norms), n, 0.0, p(P), s),
        L.dvt_video_threshold_mask(p(P), n, m, 4, 1.0, 0.0, 0.0, p(u8), s),                     # column outside P
        L.dvt_video_threshold_mask(p(P), n, m, 0, 1.0, 0.0, 0.0, None, s),
        L.dvt_video_picture_rgb(p(P), n, m, 2, p(rng), None, p(u8), s),                         # col0 + 3 > m
        L.dvt_video_picture_rgb(p(P), n, m, 0, None, None, p(u8), s),
        L.dvt_video_picture_scalar(p(P), n, m, 0, 0, 1.0, 0.0, None, 1, None, p(u8), s),        # no table
        L.dvt_video_picture_labels(p(labels), n, p(table), 17, p(u8), s),
        L.dvt_video_picture_labels(p(labels), 0, p(table), 8, p(u8), s),
        L.dvt_video_resize_bicubic_u8(p(u8), 1, 8, 8, p(u8), 8, 8, p(i32), p(i32), 65, p(i32), p(i32), 5, p(u8), s),
        L.dvt_video_resize_bicubic_u8(p(u8), 65, 8, 8, p(u8), 8, 8, p(i32), p(i32), 5, p(i32), p(i32), 5, p(u8), s),
        L.dvt_video_resize_bicubic_u8(p(u8), 1, 8, 8, p(u8), 8, 8, None, p(i32), 5, p(i32), p(i32), 5, p(u8), s),
        L.dvt_video_denorm_u8(p(x), 0, 8, p(norms), p(norms), p(u8), s),
    ]
    torch.cuda.synchronize()
    assert bad == [-1] * len(bad), bad
    assert bool((P == 5).all() and (norms == 5).all() and (labels == 5).all() and (rng == 5).all() and (u8 == 5).all())
    # and the good twin of the first call works
    assert L.dvt_video_apply(p(x), n, c, p(M[:, :4].contiguous()), m, None, 0, p(P), p(norms), None, s) == 0
    torch.cuda.synchronize()
    got = P.view(-1)[: n * m].view(n, m).cpu().double()
    assert torch.allclose(got, x.cpu().double() @ M[:, :4].cpu().double(), atol=1e-4)
    assert C.sizeof(C.c_int) == 4
