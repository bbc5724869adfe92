"""CPU: the host pieces of the segmentation evaluation (dvt_amd.seg) -- LR schedule, slide-window grid, centre padding,
metrics, checkpoint layout -- against restatements of mmcv / mmseg 0.27, and the C ABI of the head."""
import ctypes as C

import numpy as np
import pytest

from tests import seg_reference as ref


def test_poly_lr_with_linear_warmup():
    from dvt_amd.seg import poly_lr
    base, T, wu, ratio = 1e-3, 40000, 1500, 1e-6
    for it in (0, 1, 1499, 1500, 20000, 39999):
        regular = base * (1 - it / T)
        want = regular * (1 - (1 - it / wu) * (1 - ratio)) if it < wu else regular
        assert poly_lr(it, base, T) == pytest.approx(want, rel=1e-12, abs=0)
    assert poly_lr(0, base, T) == pytest.approx(base * ratio)
    assert poly_lr(1500, base, T) == pytest.approx(base * (1 - 1500 / T))


@pytest.mark.parametrize("H,W,want", [
    (512, 512, [(0, 512, 0, 512)]),                        # image equal to the crop
    (300, 400, [(0, 300, 0, 400)]),                        # smaller than the crop
    (512, 683, [(0, 512, 0, 512), (0, 512, 171, 683)]),    # the VOC-typical test size
    (512, 2100, [(0, 512, x1, x1 + 512) for x1 in (0, 341, 682, 1023, 1364, 1588)]),  # aspect above 4
])
def test_slide_windows(H, W, want):
    from dvt_amd.seg import slide_windows
    got = slide_windows(H, W)
    assert got == want
    cover = np.zeros((H, W), int)
    for y1, y2, x1, x2 in got:
        cover[y1:y2, x1:x2] += 1
    assert cover.min() >= 1


def test_center_pad():
    from dvt_amd.seg import center_pad
    assert center_pad(512, 14) == (3, 3)
    assert center_pad(518, 14) == (0, 0)
    assert center_pad(171, 14) == (5, 6)


def test_metrics_against_numpy_restatement():
    from dvt_amd.seg import total_area_to_metrics
    rng = np.random.RandomState(0)
    K = 6
    tot = np.zeros((4, K), np.int64)
    for reduce_zero in (False, True):
        tot[:] = 0
        for _ in range(3):
            label = rng.randint(0, 5, (20, 30)).astype(np.uint8)  # classes 5 never appear in the label ...
            label[:2] = 255
            pred = rng.randint(0, 4, (20, 30))                     # ... nor in the prediction (also 4 with reduce)
            ai, au, ap, al = ref.intersect_and_union(pred, label, K, reduce_zero=reduce_zero)
            tot += np.stack([ai, au, ap, al])
        got = total_area_to_metrics(np.stack([tot[0], tot[2], tot[3]]))
        want = ref.metrics(*tot)
        assert np.isnan(got["IoU"][5]) and np.isnan(want["IoU"][5])
        np.testing.assert_allclose(got["IoU"], want["IoU"], rtol=1e-12)
        np.testing.assert_allclose(got["Acc"], want["Acc"], rtol=1e-12)
        for k in ("aAcc", "mIoU", "mAcc"):
            assert got[k] == pytest.approx(want[k], rel=1e-12)
        assert np.isfinite(got["mIoU"])


def test_state_dict_names_and_shapes():
    from dvt_amd.seg import state_dict_shapes
    sd = state_dict_shapes(768, 21)
    assert sd["decode_head.conv_seg.weight"] == (21, 768, 1, 1)
    assert set(sd) == {"decode_head.conv_seg.weight", "decode_head.conv_seg.bias", "decode_head.bn.weight",
                       "decode_head.bn.bias", "decode_head.bn.running_mean", "decode_head.bn.running_var",
                       "decode_head.bn.num_batches_tracked"}


def test_seg_abi_layout_and_bad_arguments(built_lib):
    from dvt_amd import seg  # noqa: F401  (registers the signatures)
    out = (C.c_int64 * 5)()
    assert built_lib.dvt_seg_param_offsets(768, 21, out) == 0
    o = list(out)
    assert o == [0, 21 * 768, 21 * 768 + 24, 21 * 768 + 24 + 768, 21 * 768 + 24 + 2 * 768]
    assert all(v % 4 == 0 for v in o)
    assert built_lib.dvt_seg_param_offsets(770, 21, out) < 0     # C % 64
    assert built_lib.dvt_seg_param_offsets(768, 257, out) < 0    # K > 256
    assert built_lib.dvt_seg_stats_parts(2 * 37 * 37) == (2 * 37 * 37 + 127) // 128
    assert built_lib.dvt_seg_workspace_bytes(2, 37, 37, 768, 21, 512, 512) > 0
    assert built_lib.dvt_seg_workspace_bytes(0, 37, 37, 768, 21, 512, 512) < 0
    assert built_lib.dvt_seg_train_step(None, None, None, None, None, None, 1, 1, 1, 64, 2, 1, 1, 0.1, 1e-5, None, 0,
                                        None, None) < 0
    assert built_lib.dvt_seg_slide_accum(1, 2, 2, 3, 4, 4, 1, 0, 1, 1, 4, 4, None) < 0  # crop beyond the canvas
