"""Host-side pins of the device evaluation chain (supervised_dispnet_amd/evaluation.py): the zoom's number
contract against scipy, the numpy-median rule the errors kernel implements, the flags of eval_disp.py, the ragged packing."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import eval_zoom as Z  # noqa: E402
from supervised_dispnet_amd import evaluation as EV  # noqa: E402

KITTI_SIZES = [(375, 1242), (370, 1226), (376, 1241), (374, 1238)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("k", range(len(Z.SHAPE_PAIRS)))
def test_zoom_restatement_equals_scipy_bit_for_bit(k):
    from scipy.ndimage import zoom
    (h, w), (H, W) = Z.SHAPE_PAIRS[k]
    a = Z.smooth_positive_map(h, w, seed=k)
    want = zoom(a, (H / h, W / w))
    got = Z.zoom3(a, (H, W))
    assert want.shape == got.shape == (H, W) and want.dtype == got.dtype == np.float32
    assert np.array_equal(bits(want), bits(got)), int((bits(want) != bits(got)).sum())
    # scipy's zero row / column: the last source coordinate rounds above n - 1
    if ((h, w), (H, W)) == ((128, 416), (375, 1242)):
        assert np.all(want[374] == 0) and np.all(got[374] == 0) and np.all(want[373] != 0)
    if ((h, w), (H, W)) == ((256, 352), (480, 640)):
        assert np.all(want[:, 639] == 0) and np.all(got[:, 639] == 0) and np.all(want[:, 638] != 0)


@pytest.mark.parametrize("n", [1, 2, 3, 8, 9, 8960, 8961])
def test_numpy_median_rule(n):
    r = np.random.default_rng(n)
    g = r.uniform(1.0, 80.0, n).astype(np.float32)
    p = (g * r.uniform(0.5, 1.5, n)).astype(np.float32)
    if n >= 8:
        g[:3] = g[3]                                  # ties around the selected rank must not matter
    for a in (g, p):
        want = np.median(a)
        assert want.dtype == np.float32
        assert bits(EV.numpy_median_f32(a)) == bits(want)
    want = np.median(g) / np.median(p)
    assert want.dtype == np.float32 and bits(EV.median_scale_f32(g, p)) == bits(want)


def test_numpy_median_of_nothing_is_nan():
    assert np.isnan(EV.numpy_median_f32(np.zeros(0, np.float32)))


def test_parser_flags():
    import eval_disp
    base = ["--network", "disp_vgg_BN", "--pretrained-dispnet", "CKPT"]
    args = eval_disp.parse_args(base)
    assert args.eval_batch == 0 and args.readers == 4
    args = eval_disp.parse_args(base + ["--eval-batch", "8", "--readers", "64"])
    assert args.eval_batch == 8 and args.readers == 16
    assert eval_disp.parse_args(base + ["--error"]).error
    with pytest.raises(SystemExit) as e:
        eval_disp.parse_args(base + ["--eval-batch", "4", "--error"])
    assert "--error" in str(e.value) and "\n" not in str(e.value)


def test_without_eval_batch_the_run_is_handed_to_the_host_chain(monkeypatch):
    """eval_batch == 0: test_disp.main gets the command line without the two flags of eval_disp.py."""
    import eval_disp
    import test_disp
    assert eval_disp.host_chain_argv(["--network", "x", "--readers", "8", "--eval-batch=0", "--error", "--eval-batch", "0", "--pic"]) == \
        ["--network", "x", "--error", "--pic"]
    seen = []
    monkeypatch.setattr(test_disp, "main", lambda argv: seen.append(argv) or "host")
    base = ["--network", "disp_vgg_BN", "--pretrained-dispnet", "CKPT"]
    assert eval_disp.main(base + ["--readers", "2"]) == "host" and seen == [base]


def test_flags_are_spelled_out_and_picked_out_by_argparse():
    """No prefix abbreviations (test_disp.py's --error and this script's --eval-batch share a prefix), and the flags' values are not
    mistaken for positional leftovers of a list-valued flag."""
    import eval_disp
    base = ["--network", "disp_vgg_BN", "--pretrained-dispnet", "CKPT"]
    with pytest.raises(SystemExit):
        eval_disp.parse_args(base + ["--read", "2"])
    argv = base + ["--img-exts", "png", "jpg", "--readers=3", "--eval-batch", "0"]
    assert eval_disp.host_chain_argv(argv) == base + ["--img-exts", "png", "jpg"]


def test_eval_disp_never_touches_the_oracle():
    """The guard of test_product_never_touches_the_oracle_and_has_no_cpu_path for the new top-level script."""
    import re
    src = open(os.path.join(ROOT, "eval_disp.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M)
    assert "from oracle" not in src and "import oracle" not in src


def test_scale_modes_follow_the_flags():
    import eval_disp
    base = ["--network", "disp_vgg_BN", "--pretrained-dispnet", "CKPT"]
    assert EV.scale_mode(eval_disp.parse_args(base)) == (EV.SCALE_NONE, 1.0)
    assert EV.scale_mode(eval_disp.parse_args(base + ["--unsupervised"])) == (EV.SCALE_MEDIAN, 1.0)
    assert EV.scale_mode(eval_disp.parse_args(base + ["--mono"])) == (EV.SCALE_MEDIAN, 1.0)
    assert EV.scale_mode(eval_disp.parse_args(base + ["--stereo"])) == (EV.SCALE_FIXED, 5.4)


def test_prefetch_keeps_the_order():
    import eval_disp

    class Squares(object):
        def __getitem__(self, i):
            return i * i

    assert list(eval_disp.prefetched(Squares(), 23, readers=3, ahead=5)) == [i * i for i in range(23)]
    assert list(eval_disp.prefetched(Squares(), 0, readers=3, ahead=5)) == []


def test_ragged_layout_and_round_trip():
    shapes = KITTI_SIZES + [KITTI_SIZES[1], (3, 5)]
    hw, off, npix, total = EV.ragged_layout(shapes)
    assert hw.dtype == np.int32 and off.dtype == np.int64 and npix.dtype == np.int32
    assert hw.tolist() == [list(s) for s in shapes]
    assert npix.tolist() == [h * w for h, w in shapes]
    # 375 * 1242 = 465750 and 3 * 5 = 15 are no multiples of the alignment: the next image starts at the next multiple
    pad = lambda n: -(-n // EV.RAGGED_ALIGN) * EV.RAGGED_ALIGN
    want, pos = [], 0
    for h, w in shapes:
        want.append(pos)
        pos += pad(h * w)
    assert off.tolist() == want and total == pos and off[1] == 465752 and total == pos
    assert all(o % EV.RAGGED_ALIGN == 0 for o in off)
    r = np.random.default_rng(0)
    arrays = [r.uniform(0, 80, s).astype(np.float32) for s in shapes]
    masks = [r.random(s) < 0.05 for s in shapes]
    flat = EV.pack_ragged(arrays, np.float32, off, total)
    fm = EV.pack_ragged(masks, np.uint8, off, total)
    assert flat.shape == fm.shape == (total,) and fm.dtype == np.uint8
    for a, m, ua, um in zip(arrays, masks, EV.unpack_ragged(flat, hw, off), EV.unpack_ragged(fm, hw, off)):
        assert np.array_equal(a, ua) and np.array_equal(m, um.astype(bool))
    assert int(fm.sum()) == sum(int(m.sum()) for m in masks)          # the gaps hold no valid pixel
