"""CPU: the references of the video-demo tests are pinned to what they restate (Pillow's bicubic resize, oracle.vit, the
reference script's own per-frame lines as recorded by tests/golden/make_video_golden.py), and the host side of
`python -m dvt_amd.video_demo` (defaults, statistics files, refusals by name)."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import video_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RESIZES = (((120, 211), (490, 854)), ((37, 37), (518, 518)), ((5, 7), (33, 20)))


def pil_resize(a, out_hw):
    return np.asarray(Image.fromarray(a).resize((out_hw[1], out_hw[0]), Image.BICUBIC))


def resize_inputs(hw):
    h, w = hw
    rng = np.random.RandomState(h * 1000 + w)
    checker = (((np.arange(h)[:, None] + np.arange(w)[None]) % 2) * 255).astype(np.uint8)
    return {"random": rng.randint(0, 256, (h, w, 3)).astype(np.uint8), "constant": np.full((h, w, 3), 201, np.uint8),
            "checkerboard": np.repeat(checker[:, :, None], 3, 2)}


# ------------------------------------------------------------------------------------------------------ 1. bicubic
@pytest.mark.parametrize("src,dst", RESIZES)
def test_restated_bicubic_equals_pillow(src, dst):
    for name, a in resize_inputs(src).items():
        want = pil_resize(a, dst)
        got = R.bicubic_resize_u8(a, dst)
        assert got.shape == want.shape
        assert np.array_equal(got, want), f"{name} {src} -> {dst}: {(got != want).sum()} bytes differ"
    assert pil_resize(resize_inputs(src)["checkerboard"], dst).max() == 255  # the overshoot is clamped, not wrapped


@pytest.mark.parametrize("src,dst", RESIZES)
def test_product_tables_equal_pillow(src, dst):
    """The tables dvt_amd.video uploads, applied in numpy exactly as the resample kernel applies them."""
    from dvt_amd import video as VD
    xb, xc = VD.bicubic_tables(src[1], dst[1])
    yb, yc = VD.bicubic_tables(src[0], dst[0])
    assert xc.shape[1] == 5 and yc.shape[1] == 5  # upsampling: support 2, ksize 5
    assert (xb[:, 0] >= 0).all() and (xb[:, 0] + xb[:, 1] <= src[1]).all() and (xb[:, 1] <= xc.shape[1]).all()
    assert (yb[:, 0] >= 0).all() and (yb[:, 0] + yb[:, 1] <= src[0]).all() and (yb[:, 1] <= yc.shape[1]).all()
    for name, a in resize_inputs(src).items():
        assert np.array_equal(R.apply_tables_u8(a, xb, xc, yb, yc), pil_resize(a, dst)), name


def test_product_tables_when_shrinking():
    from dvt_amd import video as VD
    a = resize_inputs((33, 20))["random"]
    xb, xc = VD.bicubic_tables(20, 7)
    yb, yc = VD.bicubic_tables(33, 5)
    assert np.array_equal(R.apply_tables_u8(a, xb, xc, yb, yc), pil_resize(a, (5, 7)))
    assert np.array_equal(R.bicubic_resize_u8(a, (5, 7)), pil_resize(a, (5, 7)))


# ------------------------------------------------------------------------------------------------------ 2. chunked ViT
@pytest.mark.parametrize("n_reg", (0, 4))
def test_chunked_vit_equals_oracle(n_reg):
    from dvt_amd.vit import random_state_dict
    from oracle import vit as ovit
    sd = random_state_dict(128, 2, 14, (0 if n_reg else 1) + 4 * 4, seed=3, well_conditioned=True, n_reg=n_reg)
    img = torch.randn(1, 3, 70, 126, generator=torch.Generator().manual_seed(1))
    want = ovit.forward_features(sd, img, patch=14, stride=4)
    assert tuple(want.shape) == (1, 15, 29, 128)
    for chunk in (64, 100, 10 ** 6):
        got = R.chunked_vit_forward(sd, img, 14, 4, q_chunk=chunk)
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-5), (chunk, (got - want).abs().max())


# ------------------------------------------------------------------------------------------------------ 3. the script's lines
@pytest.mark.parametrize("case", ("a", "b"))
def test_frame_restatement_equals_the_scripts_lines(case):
    g = np.load(os.path.join(GOLDEN, "video_reference.npz"))
    x = g[f"{case}.x"]
    gh, gw, c = x.shape
    v = R.frame_values(x.reshape(-1, c), g[f"{case}.instance"], g[f"{case}.dataset"], g[f"{case}.standard"], g[f"{case}.fg"],
                       g[f"{case}.fg_standard"], g[f"{case}.centers"])
    pics = R.frame_token_pictures(v, (gh, gw), int(g[f"{case}.clusters"]))
    assert 0 < v["mask_fg"].sum() < gh * gw and 0 < v["mask_standard"].sum() < gh * gw  # both masks do something
    for kind in R.MAP_KINDS:
        assert np.array_equal(pics[kind], g[f"{case}.{kind}"]), kind


def test_u8_tables_are_what_matplotlib_gives():
    import matplotlib
    from dvt_amd import video as VD
    v = np.linspace(0, 1, 4001).astype(np.float32)
    want = (matplotlib.colormaps["inferno"](v)[:, :3] * 255).astype(np.uint8)
    idx = np.minimum((v * np.float32(256)).astype(np.int64), 255)
    assert np.array_equal(VD.color_table_u8("inferno")[idx], want)
    for k in (8, 5, 3, 16):
        lab = np.arange(k).astype(np.float32)
        want = (matplotlib.colormaps["rainbow"](lab / k)[:, :3] * 255).astype(np.uint8)
        assert np.array_equal(VD.label_table_u8("rainbow", k), want)


# ------------------------------------------------------------------------------------------------------ 4. the command
def test_cli_defaults_are_the_scripts_constants():
    from dvt_amd import video as VD
    from dvt_amd import video_demo as D
    flags = json.load(open(os.path.join(GOLDEN, "video_reference_flags.json")))
    a = D.get_args(["--frames", "x", "--stats", "s.npz"])
    for k in ("model", "stride_size", "height", "width", "fps", "num_clusters", "output_dir"):
        assert getattr(a, k) == flags[k], k
    assert a.dtype == "bfloat16" and a.seed == 0 and a.stats_prefix == "denoised" and not a.allow_random_vit
    assert VD.NORM_TEMPERATURE == flags["norm_temperature"] and VD.FG_THRESHOLD == flags["fg_threshold"]
    assert D.get_args(["--frames", "a", "--frames", "b", "--stats", "s"]).frames == ["a", "b"]
    assert len(VD.KINDS) == 10 and set(VD.VIDEO_NAMES) == set(VD.KINDS)
    assert VD.VIDEO_NAMES["input"] == "image" and VD.VIDEO_NAMES["pca_instance"] == "instance_pca"


def test_stats_npz_and_pth(tmp_path):
    from dvt_amd import _lib
    from dvt_amd import video as VD
    npz = os.path.join(GOLDEN, "video_stats.npz")
    s = VD.load_stats(npz)
    assert s["reduct_mat_full"].shape == (768, 3) and s["standard_mapping"].shape == (768, 1)
    raw = np.load(npz)
    pth = str(tmp_path / "stats.pth")
    torch.save({k: torch.from_numpy(raw[k]) for k in raw.files}, pth)
    for prefix in ("denoised", "dinov2"):
        a, b = VD.load_stats(npz, prefix), VD.load_stats(pth, prefix)
        assert np.array_equal(a["reduct_mat_full"], raw[f"{prefix}_reduct_mat_full"])
        assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(VD.load_stats(npz, "dinov2")["reduct_mat_full"], s["reduct_mat_full"])
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, denoised_reduct_mat_full=raw["denoised_reduct_mat_full"])
    with pytest.raises(_lib.DvtError, match="denoised_standard_mapping"):
        VD.load_stats(bad)
    with pytest.raises(_lib.DvtError, match="does not exist"):
        VD.load_stats(str(tmp_path / "none.npz"))
    import pickle
    evil = str(tmp_path / "evil.pth")  # weights_only=True: a pickle that is not plain tensors is refused, not executed
    torch.save({"denoised_reduct_mat_full": np.random.RandomState}, evil)
    with pytest.raises((pickle.UnpicklingError, RuntimeError)):
        VD.load_stats(evil)


def test_refusals_by_name(built_lib, tmp_path):
    from dvt_amd import _lib
    from dvt_amd import video as VD
    from dvt_amd import video_demo as D
    scene = os.path.join(GOLDEN, "davis-mallard-water")
    stats = os.path.join(GOLDEN, "video_stats.npz")
    out = str(tmp_path / "out")
    base = ["--frames", scene, "--stats", stats, "--output_dir", out, "--allow_random_vit"]
    todo = D.plan(D.get_args(base))
    assert todo["grid_hw"] == (120, 211) and todo["channels"] == 768  # from the extractor's configuration
    assert [os.path.basename(f) for f in todo["scenes"][0][1]] == ["00000.jpg", "00040.jpg"]
    assert todo["scenes"][0][0] == "davis-mallard-water"
    cases = ((["--stride_size", "2"], "DVT_VIS_MAX_ROWS"),                       # 239 x 421 tokens
             (["--model", "vit_small_patch14_dinov2.lvd142m"], "channels"),      # stats made for 768
             (["--num_clusters", "17"], "DVT_VIS_MAX_K"),
             (["--frames", str(tmp_path / "nowhere")], "not a directory"),
             (["--vit_checkpoint", str(tmp_path / "none.pth")], "does not exist"))
    for extra, word in cases:
        with pytest.raises(_lib.DvtError, match=word):
            D.plan(D.get_args(base + extra))
    with pytest.raises(_lib.DvtError, match="no ViT weights"):
        D.plan(D.get_args(base[:-1]))
    with pytest.raises(_lib.DvtError, match="multiple of 64"):
        VD.check_geometry((10, 10), 96)
    assert not os.path.exists(out)  # refused before anything is written
    with pytest.raises(_lib.DvtError, match="HIP device"):
        VD.VideoDemoEngine("cpu", (4, 4), 64, (8, 8), {"reduct_mat_full": np.zeros((64, 3), np.float32),
                                                       "standard_mapping": np.zeros((64, 1), np.float32)})
