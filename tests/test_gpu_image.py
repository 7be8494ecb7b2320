"""csrc/dn_image.hip on the GPU: dn_imresize_u8 against kitti_eval.imresize_bilinear (byte-scale + Pillow's
bilinear resize) and dn_u8_normalize_flip, dn_colorize_u8 against utils.tensor2array, dn_contrast_u8 against PIL -- every byte equal."""
import ctypes
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
import supervised_dispnet_amd.utils as U  # noqa: E402
from supervised_dispnet_amd import _lib, inference, kitti_eval as KE  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
NORMS = [([0.5, 0.5, 0.5], [0.5, 0.5, 0.5]), ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])]


@pytest.fixture(scope="module")
def ops():
    return inference.ImageOps(DEV)


def _frame(H, W, lo, hi, seed):
    a = np.random.RandomState(seed).randint(lo, hi + 1, (H, W, 3))
    a.flat[0], a.flat[1] = lo, hi
    return a.astype(np.uint8)


def _want(frame, h, w):
    """What the reference feeds the network: the frame itself when it has the size, else scipy.misc.imresize of the float frame."""
    if frame.shape[:2] == (h, w):
        return frame
    return KE.imresize_bilinear(frame.astype(np.float32), (h, w))


def _normalised(u8, mean, std):
    B, h, w, _ = u8.shape
    out = torch.empty((B, 3, h, w), dtype=torch.float32, device=DEV)
    d_mean, d_std = torch.tensor(mean, device=DEV), torch.tensor(std, device=DEV)
    _lib.call("dn_u8_normalize_flip", u8.data_ptr(), None, B, h, w, 3, d_mean.data_ptr(), d_std.data_ptr(), (ctypes.c_float * 3)(*mean),
              (ctypes.c_float * 3)(*std), out.data_ptr(), 3 * h * w, h * w, torch.cuda.current_stream().cuda_stream)
    return out


def _check(ops, frames, h, w):
    for mean, std in NORMS:
        u8, f32 = ops.imresize(frames, (h, w), mean, std, want_u8=True)
        got = u8.cpu().numpy()
        for b, f in enumerate(frames):
            want = _want(f, h, w)
            bad = int((got[b] != want).sum())
            print("frame %d %s -> %s: %d bytes differ" % (b, f.shape[:2], (h, w), bad))
            assert bad == 0
        assert torch.equal(f32.view(torch.int32), _normalised(u8, mean, std).view(torch.int32))
    only_u8, none = ops.imresize(frames, (h, w), want_u8=True)          # either output alone
    assert none is None and torch.equal(only_u8, u8)
    none, only_f32 = ops.imresize(frames, (h, w), *NORMS[1])
    assert none is None and torch.equal(only_f32.view(torch.int32), f32.view(torch.int32))


def test_imresize_ragged_batch(ops):
    """37x53 shrinks, 9x13 grows, 40x24 skips the horizontal pass, 16x24 is passed through (a byte-scale applied by mistake would stretch
    its 40 ... 200), 33x90 is low-contrast and 7x24 skips the horizontal pass while it grows."""
    frames = [_frame(37, 53, 0, 255, 1), _frame(9, 13, 0, 255, 2), _frame(40, 24, 0, 255, 3), _frame(16, 24, 40, 200, 4),
              _frame(33, 90, 90, 130, 5), _frame(7, 24, 3, 250, 6), np.full((21, 30, 3), 77, np.uint8)]
    _check(ops, frames, 16, 24)
    assert not _want(frames[6], 16, 24).any()                           # a constant frame becomes 0


def test_imresize_kitti_sizes(ops):
    """The real tap count (6 and 6), a 16 x 7 tile grid with a ragged right edge, two sizes in one batch."""
    _check(ops, [_frame(375, 1242, 0, 255, 7), _frame(370, 1226, 10, 240, 8)], 128, 416)


def test_imresize_many_taps_and_odd_width(ops):
    """33 -> 5 rows is 14 taps; 19 output columns take dn_u8_normalize_flip's general path in the comparison; 140 -> 9 rows is the bound of 32 taps and needs
    more source rows than the kernel stages at once (the tile's output rows go in groups)."""
    _check(ops, [_frame(33, 7, 0, 255, 9)], 5, 19)
    _check(ops, [_frame(140, 40, 0, 255, 10), _frame(9, 19, 0, 255, 11)], 9, 19)


def test_imresize_refuses_more_taps_than_its_bound(ops):
    assert inference.resize_coefficients(200, 5)[2].shape[1] > inference.MAX_TAPS
    with pytest.raises(_lib.DispnetHipError, match="taps"):
        ops.imresize([_frame(200, 8, 0, 255, 12)], (5, 8), want_u8=True)
    with pytest.raises(ValueError, match="frame 1.*uint8"):
        ops.imresize([_frame(9, 9, 0, 255, 13), np.zeros((9, 9), np.uint8)], (5, 8), want_u8=True)


RECT = (3, 17, 5, 42)                                                   # not tile-aligned, inside 19 x 45


def _maps():
    r = np.random.RandomState(20)
    x = r.uniform(0.0, 12.0, (2, 19, 45)).astype(np.float32)            # values above 10
    x[1] *= 0.3
    z = x.copy()
    z[0, 5, 7] = z[1, 16, 41] = z[1, 3, 5] = 0.0                        # 1 / 0 = inf inside the rectangle
    return x, z


@pytest.mark.parametrize("mode", ["table", "grey"])
def test_colorize_against_tensor2array(ops, mode):
    table = np.random.RandomState(21).randint(0, 256, (256, 3)).astype(np.uint8) if mode == "table" else None
    has_reference = table is not None or U.colour_table("bone") is None  # with OpenCV tensor2array has no grey branch
    x, z = _maps()
    r0, r1, c0, c1 = RECT
    cases = [(x, RECT, None, False), (x, RECT, 10, False), (x, None, None, False), (z, RECT, 10, True), (z, None, 10, True),
             (x, RECT, None, True)]
    for maps, rect, max_value, recip in cases:
        got = ops.colorize(torch.from_numpy(maps).to(DEV), rect, max_value, table, reciprocal=recip).cpu().numpy()
        for b in range(2):
            t = torch.from_numpy(maps[b].copy())
            t = 1 / t if recip else t
            t = t if rect is None else t[r0:r1, c0:c1]
            assert np.array_equal(got[b], PR.colorize(t.numpy(), max_value, table))
            if has_reference:
                arr = U.tensor2array(t[None], max_value=max_value, colormap="bone", channel_first=False, table=table)
                assert np.array_equal(got[b], (255 * arr).astype(np.uint8)), (rect, max_value, recip, b)
    # the per-image maximum of a map with an inf is inf: finite values give 0 and inf / inf is a NaN, which the kernel defines as 0
    got = ops.colorize(torch.from_numpy(z).to(DEV), RECT, None, table, reciprocal=True).cpu().numpy()
    zero = np.broadcast_to(table[0] if table is not None else np.zeros(3, np.uint8), got.shape)
    assert np.array_equal(got, zero)
    assert np.array_equal(inference.colorize(torch.from_numpy(x).to(DEV), RECT, 10, table).cpu().numpy(),
                          ops.colorize(torch.from_numpy(x).to(DEV), RECT, 10, table).cpu().numpy())
    with pytest.raises(_lib.DispnetHipError, match="rectangle"):
        ops.colorize(torch.from_numpy(x).to(DEV), (3, 20, 5, 42), 10, table)


def test_contrast_against_pil(ops):
    from PIL import Image, ImageEnhance
    r = np.random.RandomState(22)
    ims = np.stack([r.randint(0, 256, (21, 37, 3)), r.randint(0, 256, (21, 37, 3)) // 4 + 100, np.full((21, 37, 3), 77)]).astype(np.uint8)
    for factor in (4.0, 0.5):
        got = ops.contrast(torch.from_numpy(ims).to(DEV), factor).cpu().numpy()
        for b in range(3):
            want = np.asarray(ImageEnhance.Contrast(Image.fromarray(ims[b])).enhance(factor))
            assert np.array_equal(got[b], want), (factor, b)
