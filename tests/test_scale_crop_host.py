"""Host side of the random scale-and-crop augmentation, no GPU: the numpy restatement of tests/scale_crop.py
against Pillow itself, the host chain data.Transform(scale_crop=True) against the restatement, the order of the draws, the windowed
coefficient tables the kernels read, and train.py's flag."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import pil_resize as PR  # noqa: E402
import scale_crop as SC  # noqa: E402
from supervised_dispnet_amd import data as D  # noqa: E402

SIZES = [(24, 40), (128, 416)]


def _scaled_sizes(H, W):
    return [(H, W), (H, int(1.07 * W)), (int(1.07 * H), W), (int(1.15 * H), int(1.15 * W))]


def _frame(H, W, seed):
    r = np.random.RandomState(seed)
    return r.randint(30, 230, (H, W, 3)).astype(np.uint8)          # min > 0, max < 255: the byte-scale moves every value


def _depth(H, W, seed, density=0.3):
    r = np.random.RandomState(seed)
    return (r.rand(H, W) * 80 * (r.rand(H, W) < density)).astype(np.float32)


@pytest.mark.parametrize("H,W", SIZES)
def test_restatement_equals_pillow(H, W):
    """Byte-scale, Image.resize(BILINEAR) of the whole frame ('RGB') and depth ('L'), crop: every byte equal, for the four kinds of
    scaled size and the two extreme offsets."""
    from PIL import Image
    frame, d = _frame(H, W, H), _depth(H, W, W)
    for sh, sw in _scaled_sizes(H, W):
        want_rgb = np.asarray(Image.fromarray(PR.bytescale(frame.astype(np.float32)), "RGB").resize((sw, sh), Image.BILINEAR))
        want_l = np.asarray(Image.fromarray(PR.bytescale(d), "L").resize((sw, sh), Image.BILINEAR))
        got_rgb, got_l = SC.scaled_u8(frame.astype(np.float32), sh, sw), SC.scaled_u8(d, sh, sw)
        assert got_rgb.shape == (sh, sw, 3) and got_l.shape == (sh, sw)
        for oy, ox in {(0, 0), (sh - H, sw - W)}:
            assert np.array_equal(got_rgb[oy:oy + H, ox:ox + W], want_rgb[oy:oy + H, ox:ox + W]), (sh, sw, oy, ox)
            assert np.array_equal(got_l[oy:oy + H, ox:ox + W], want_l[oy:oy + H, ox:ox + W]), (sh, sw, oy, ox)
            u8, _ = SC.image(frame, False, sh, sw, oy, ox, (0.5,) * 3, (0.5,) * 3)
            assert np.array_equal(u8, want_rgb[oy:oy + H, ox:ox + W])
            got_d = SC.depth(d, False, sh, sw, oy, ox)
            want_d = (want_l[oy:oy + H, ox:ox + W].astype(np.float64) / 255.0 * np.float64(d.max())).astype(np.float32)
            assert got_d.dtype == np.float32 and np.array_equal(got_d, want_d)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("flip", [False, True])
def test_host_chain_equals_restatement(H, W, flip):
    """data.Transform(scale_crop=True).apply for fixed draws: images, depth and intrinsics, flipped and not."""
    mean, std = D.normalization(imagenet=True)
    t = D.Transform(mean, std, flip=True, scale_crop=True)
    frames = [_frame(H, W, 10 + i) for i in range(3)]
    frames[2][:] = 77                                               # a constant frame: scale 1
    k = np.array([[241.67, 0, 204.17], [0, 246.28, 59.0], [0, 0, 1]], dtype=np.float32)
    for i, (sh, sw) in enumerate(_scaled_sizes(H, W)):
        d = _depth(H, W, 20 + i, density=0.0 if i == 0 else 0.05)   # an all-zero map, then sparse ones
        sx, sy = 1.0 + 0.15 * i / 3, 1.0 + 0.11 * i / 3
        for oy, ox in {(0, 0), (sh - H, sw - W), ((sh - H) // 2, (sw - W) // 3)}:
            imgs, gt, kk = t.apply([f.astype(np.float32) for f in frames], d, k, flip, (sx, sy, sh, sw, oy, ox))
            for f, got in zip(frames, imgs):
                _, want = SC.image(f, flip, sh, sw, oy, ox, mean, std)
                assert got.dtype == torch.float32 and np.array_equal(got.numpy().view(np.int32), want.view(np.int32)), (sh, sw, oy, ox)
            assert gt.dtype == torch.float32
            assert np.array_equal(gt.numpy().view(np.int32), SC.depth(d, flip, sh, sw, oy, ox).view(np.int32)), (sh, sw, oy, ox)
            want_k = SC.intrinsics(k, W, flip, sx, sy, oy, ox)
            assert kk.dtype == np.float32 and np.array_equal(kk.view(np.int32), want_k.view(np.int32))
    assert np.array_equal(k, np.array([[241.67, 0, 204.17], [0, 246.28, 59.0], [0, 0, 1]], dtype=np.float32))      # the caller's copy is intact


def test_transform_without_the_flag_is_unchanged():
    """scale_crop=False: the same draws consumed (none from numpy.random) and the same values as the chain without the argument."""
    import random
    mean, std = D.normalization()
    frame, d = _frame(24, 40, 1).astype(np.float32), _depth(24, 40, 2)
    k = np.eye(3, dtype=np.float32)
    np.random.seed(5)
    state = np.random.get_state()[1].copy()
    random.seed(3)
    a = D.Transform(mean, std, True)([frame], d, k)
    random.seed(3)
    b = D.Transform(mean, std, True, scale_crop=False)([frame], d, k)
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(np.random.get_state()[1], state)


def test_draw_order():
    """The loader-side draw function consumes a RandomState exactly as the reference's four numpy calls do, x scale first."""
    for H, W, seed in [(128, 416, 0), (24, 37, 7), (20, 70, 123)]:
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        for _ in range(50):
            sx, sy, sh, sw, oy, ox = D.draw_scale_crop(a, H, W)
            x_scaling, y_scaling = b.uniform(1, 1.15, 2)
            scaled_h, scaled_w = int(H * y_scaling), int(W * x_scaling)
            offset_y = b.randint(scaled_h - H + 1)
            offset_x = b.randint(scaled_w - W + 1)
            assert (sx, sy, sh, sw, oy, ox) == (x_scaling, y_scaling, scaled_h, scaled_w, offset_y, offset_x)
            assert H <= sh <= int(1.15 * H) and W <= sw <= int(1.15 * W) and 0 <= oy <= sh - H and 0 <= ox <= sw - W
        assert a.randint(1 << 30) == b.randint(1 << 30)             # and nothing more
    # the global generator, as data.Transform draws
    np.random.seed(11)
    got = D.draw_scale_crop(np.random, 128, 416)
    assert got == SC.draws(np.random.RandomState(11), 128, 416)


@pytest.mark.parametrize("n", [24, 37, 40, 70, 128, 416])
def test_windowed_tables(n):
    """Rows [o0, o0 + n) of the table of the axis n -> O equal tests/pil_resize.coefficients(n, O)[o0:o0 + n]; O == n is the identity."""
    from supervised_dispnet_amd import inference as I
    for O in sorted({n + 1, n + 2, int(1.07 * n), int(1.15 * n)}):
        want = PR.coefficients(n, O)
        for o0 in sorted({0, (O - n) // 2, O - n}):
            rows, taps = I.scale_crop_rows(n, O, o0)
            assert rows.shape == (n, 4) and rows.dtype == np.int32 and taps <= I.SCALE_CROP_TAPS
            for r, (first, k) in zip(rows, want[o0:o0 + n]):
                assert len(k) <= 3 and r[0] == first and list(r[1:1 + len(k)]) == list(k) and not r[1 + len(k):].any()
            assert taps == max(len(k) for _, k in want)
    rows, taps = I.scale_crop_rows(n, n, 0)
    assert taps == 1 and np.array_equal(rows, np.stack([np.arange(n), np.full(n, 1 << 22), np.zeros(n), np.zeros(n)], 1))
    with pytest.raises(ValueError):
        I.scale_crop_rows(n, n - 1, 0)
    with pytest.raises(ValueError):
        I.scale_crop_rows(n, n + 4, 5)
    table, taps = I.scale_crop_table(n, 2 * n, [(n + 3, 2 * n, 1, 0), (n, 2 * n + 5, 0, 5)])
    assert table.shape == (2, 3 * n, 4) and taps <= 3
    assert np.array_equal(table[0, 2 * n:], I.scale_crop_rows(n, n + 3, 1)[0]) and np.array_equal(table[1, :2 * n], I.scale_crop_rows(2 * n, 2 * n + 5, 5)[0])


def test_train_flag():
    import train
    p = train.build_parser()
    assert p.get_default("scale_crop") is False
    assert p.parse_args(["DIR"]).scale_crop is False and p.parse_args(["DIR", "--scale-crop"]).scale_crop is True
    for extra in (["--dataset", "nyu", "--with-gt"], ["--synthetic", "8"], ["--synthetic", "8", "--dataset", "nyu"]):
        with pytest.raises(SystemExit) as e:
            train.check_dataset_args(p.parse_args(["DIR", "--scale-crop"] + extra))
        assert "--scale-crop" in str(e.value) and "\n" not in str(e.value)
        train.check_dataset_args(p.parse_args(["DIR"] + extra))     # without the flag these settings pass
    train.check_dataset_args(p.parse_args(["DIR", "--scale-crop", "--shards", "S", "--unsupervised"]))
