"""monodepth2's colour jitter on the host (no GPU): the numpy restatement of tests/colour_jitter.py against the
installed Pillow -- every colour through both HSV conversions, the three enhancers on random frames --, data.colour_jitter_u8 (Pillow
itself, the oracle of tests/test_gpu_colour_jitter.py) against the restatement on the cases the GPU tests use, the draw order of
data.draw_colour_jitter, data.Transform(color_aug=True) against the manual chain, the scene-folder batch through train._to_device_batch, and train.py's refusals."""
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from PIL import Image  # noqa: E402

import colour_jitter as CJ  # noqa: E402
from supervised_dispnet_amd import data as D  # noqa: E402


@pytest.fixture(scope="module")
def colours():
    return CJ.all_colours()


def _pil_hue(a, shift):
    h, s, v = Image.fromarray(a).convert("HSV").split()
    nh = ((np.asarray(h, dtype=np.int32) + shift) % 256).astype(np.uint8)
    return np.asarray(Image.merge("HSV", (Image.fromarray(nh), s, v)).convert("RGB"))


def test_hsv_conversions_equal_pillow_on_every_colour(colours):
    want = np.asarray(Image.fromarray(colours).convert("HSV"))
    assert np.array_equal(CJ.rgb_to_hsv(colours), want)
    # ... and back from every (H, S, V) triple, reachable from an RGB colour or not
    want = np.asarray(Image.frombytes("HSV", (4096, 4096), colours.tobytes()).convert("RGB"))
    assert np.array_equal(CJ.hsv_to_rgb(colours), want)


@pytest.mark.parametrize("shift", [0, 231])
def test_hue_equals_pillow_on_the_all_colours_frame(colours, shift):
    got = CJ.hue(colours, shift)
    assert np.array_equal(got, _pil_hue(colours, shift))
    if shift == 0:
        assert (got != colours).any()                    # the round trip is lossy: shift 0 is no identity


def test_enhancers_equal_pillow():
    from PIL import ImageEnhance
    factors = sorted(set([0.8, 1.0, 1.2] + list(np.random.RandomState(0).uniform(0.8, 1.2, 40))))
    for k, shape in enumerate([(13, 17), (32, 48)]):
        a = CJ.random_frames(shape, 20 + k)
        im = Image.fromarray(a)
        for f in factors:
            assert np.array_equal(CJ.brightness(a, f), np.asarray(ImageEnhance.Brightness(im).enhance(f))), f
            assert np.array_equal(CJ.contrast(a, f), np.asarray(ImageEnhance.Contrast(im).enhance(f))), f
            assert np.array_equal(CJ.saturation(a, f), np.asarray(ImageEnhance.Color(im).enhance(f))), f
    flat = np.full((6, 5, 3), (12, 200, 77), dtype=np.uint8)
    assert CJ.contrast_mean(flat) == int(CJ.luma(flat)[0, 0])           # a constant frame's mean is its own luma


@pytest.mark.parametrize("H,W", [(5, 7), (8, 16)])
def test_colour_jitter_u8_equals_the_restatement_in_every_order(H, W):
    frames = CJ.random_frames((24, H, W), 100 * H + W)
    for f, p in zip(frames, CJ.order_params()):
        assert np.array_equal(D.colour_jitter_u8(f, p), CJ.jitter(f, p)), p
    assert np.array_equal(D.colour_jitter_u8(frames[0], None), frames[0])
    assert np.array_equal(D.colour_jitter_u8(frames[0].astype(np.float32), CJ.order_params()[5]), CJ.jitter(frames[0], CJ.order_params()[5]))


def test_colour_jitter_u8_on_degenerate_and_ragged_frames():
    for frame in CJ.degenerate_frames(6, 10):
        for shift in (0, 1, 128, 255):
            for order in ((3, 0, 1, 2), (1, 2, 3, 0)):
                p = (order, 1.1, 0.9, 1.15, shift)
                assert np.array_equal(D.colour_jitter_u8(frame, p), CJ.jitter(frame, p)), (frame[0, 0], p)
    for shape, seed in (((3, 23, 37), 1), ((1, 40, 136), 2)):
        for f, p in zip(CJ.random_frames(shape, seed), CJ.order_params(seed)[7:]):
            assert np.array_equal(D.colour_jitter_u8(f, p), CJ.jitter(f, p)), p


class _Scripted(object):
    """a generator that returns given values and counts the calls"""

    def __init__(self, u, h):
        self.u, self.h, self.calls = u, h, []

    def random_sample(self):
        self.calls.append("random_sample")
        return self.u

    def permutation(self, n):
        self.calls.append("permutation")
        return np.array([2, 0, 3, 1])

    def uniform(self, lo, hi):
        self.calls.append("uniform(%g, %g)" % (lo, hi))
        return self.h if lo < 0 else 0.5 * (lo + hi)


def test_draw_colour_jitter():
    want = ["random_sample", "permutation", "uniform(0.8, 1.2)", "uniform(0.8, 1.2)", "uniform(0.8, 1.2)", "uniform(-0.1, 0.1)"]
    for u, h, shift in ((0.7, 0.05, 12), (0.7, -0.05, 256 - 12), (0.7, -0.001, 0), (0.7, 0.1, 25), (0.7, -0.1, 256 - 25)):
        rng = _Scripted(u, h)
        order, b, c, s, got = D.draw_colour_jitter(rng)
        assert rng.calls == want and order == (2, 0, 3, 1) and (b, c, s) == (1.0, 1.0, 1.0)
        assert got == shift == int(np.uint8(np.int64(h * 255) % 256))
    for u in (0.5, 0.2):                                 # jittered iff u > 0.5; the other five calls are made all the same
        rng = _Scripted(u, 0.05)
        assert D.draw_colour_jitter(rng) is None and rng.calls == want
    # on a real generator: the state after n draws does not depend on how many of them were jittered
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    got = [D.draw_colour_jitter(a) for _ in range(64)]
    for _ in range(64):
        b.random_sample(), b.permutation(4), b.uniform(0.8, 1.2), b.uniform(0.8, 1.2), b.uniform(0.8, 1.2), b.uniform(-0.1, 0.1)
    assert a.random_sample() == b.random_sample()
    n = sum(p is not None for p in got)
    assert 16 < n < 48
    for p in got:
        if p is not None:
            assert sorted(p[0]) == [0, 1, 2, 3] and all(0.8 <= f <= 1.2 for f in p[1:4]) and (p[4] <= 25 or p[4] >= 231)


@pytest.mark.parametrize("scale_crop", [False, True], ids=["flip", "flip+scale_crop"])
def test_transform_applies_the_jitter_in_front_of_the_existing_chain(scale_crop):
    mean, std = D.normalization(imagenet=True)
    H, W = 12, 20
    frames = [f.astype(np.float32) for f in CJ.random_frames((3, H, W), 5)]
    gt = np.random.RandomState(1).rand(H, W).astype(np.float32) * 50
    k = np.array([[10, 0, 9.5], [0, 11, 6.5], [0, 0, 1]], dtype=np.float32)
    t = D.Transform(mean, std, flip=True, scale_crop=scale_crop, color_aug=True, keep_plain=True)
    plain_t = D.Transform(mean, std, flip=True, scale_crop=scale_crop)
    jittered = 0
    for seed in range(8):
        random.seed(seed)
        np.random.seed(seed)
        imgs, g, kk = t(frames, gt, k.copy())
        random.seed(seed)
        np.random.seed(seed)
        flip = random.random() < 0.5
        params = D.draw_colour_jitter(np.random)
        crop = D.draw_scale_crop(np.random, H, W) if scale_crop else None
        want, wg, wk = plain_t.apply([D.colour_jitter_u8(f, params).astype(np.float32) for f in frames], gt, k.copy(), flip, crop)
        wplain = plain_t.apply(frames, gt, k.copy(), flip, crop)[0]
        assert len(imgs) == 6
        for a, b in zip(imgs, want + wplain):
            assert torch.equal(a, b)
        assert torch.equal(g, wg) and np.array_equal(kk, wk)
        jittered += params is not None
        if params is None:
            assert all(torch.equal(a, b) for a, b in zip(imgs[:3], imgs[3:]))
    assert 0 < jittered < 8
    # without keep_plain: the jittered frames only; without color_aug: no draw from numpy.random
    random.seed(0)
    np.random.seed(0)
    assert len(D.Transform(mean, std, flip=True, color_aug=True)(frames, gt, k.copy())[0]) == 3
    np.random.seed(0)
    state = np.random.get_state()[1].copy()
    assert len(plain_t(frames, gt, k.copy())[0]) == 3
    assert scale_crop or np.array_equal(np.random.get_state()[1], state)


def test_sequence_folder_carries_the_plain_frames(tmp_path):
    from tests.cases import make_scene_folders
    root = make_scene_folders(tmp_path / "kitti", frames=5, h=16, w=24)
    mean, std = D.normalization()
    base = D.SequenceFolder(str(root), seed=0, transform=D.Transform(mean, std, flip=True), with_refs=True)
    aug = D.SequenceFolder(str(root), seed=0, transform=D.Transform(mean, std, flip=True, color_aug=True, keep_plain=True), with_refs=True)
    seen = 0
    for i in range(len(base)):
        random.seed(i)
        np.random.seed(i)
        a = base[i]
        random.seed(i)
        np.random.seed(i)
        b = aug[i]
        assert len(a) == 5 and len(b) == 6 and len(b[5]) == 1 + len(b[1])
        assert torch.equal(b[5][0], a[0]) and all(torch.equal(x, y) for x, y in zip(b[5][1:], a[1]))       # the same flip: plain == the old sample
        assert np.array_equal(a[2], b[2]) and torch.equal(a[4], b[4])
        seen += not torch.equal(b[0], a[0])
    assert seen > 0


@pytest.mark.parametrize("extra,msg", [(["--dataset", "nyu", "--with-gt"], "--dataset nyu"), (["--synthetic", "8"], "--synthetic")])
def test_train_refuses_color_aug_where_there_are_no_decoded_frames(extra, msg):
    import train
    with pytest.raises(SystemExit) as e:
        train.main(["DATA", "--color-aug"] + extra)
    text = str(e.value.code)
    assert "--color-aug" in text and msg in text and "\n" not in text
    assert train.build_parser().parse_args(["DATA"]).color_aug is False


def test_scene_folder_batch_reaches_the_loss_as_plain_and_the_networks_as_jittered(tmp_path):
    """the JPEG path of --color-aug --unsupervised end to end on the host: SequenceFolder's sixth entry through the DataLoader's default
    collate and train._to_device_batch onto ._dn_plain, which train.plain_frames hands to the loss; a batch without the flag has no
    such attribute and is its own plain batch"""
    import train
    from tests.cases import make_scene_folders
    root = make_scene_folders(tmp_path / "kitti", frames=5, h=16, w=24)
    mean, std = D.normalization()
    cpu = torch.device("cpu")

    def batch(**kw):
        ds = D.SequenceFolder(str(root), seed=0, transform=D.Transform(mean, std, flip=True, **kw), with_refs=True)
        random.seed(7)
        np.random.seed(7)
        return next(iter(torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, num_workers=0)))

    raw, base = batch(color_aug=True, keep_plain=True), batch()
    assert len(raw) == 6 and len(base) == 5
    tgt, refs, k, kinv, gt = train._to_device_batch(raw, cpu, True)
    btgt, brefs, bk, bkinv, bgt = train._to_device_batch(base, cpu, True)
    ptgt, prefs = train.plain_frames(tgt, refs)
    assert tgt.shape == (4, 3, 16, 24) and len(refs) == len(prefs) == 2
    assert torch.equal(ptgt, btgt) and all(torch.equal(a, b) for a, b in zip(prefs, brefs))      # the same flips: plain == the old batch
    assert torch.equal(k, bk) and torch.equal(kinv, bkinv) and torch.equal(gt, bgt)
    assert not torch.equal(tgt, ptgt)                                                              # some sample of the four is jittered
    same = [bool(torch.equal(tgt[j], ptgt[j])) for j in range(4)]
    assert any(same) and not all(same), same                                                       # ... and some is not
    for j in range(4):                                                                             # one draw per sample: refs follow the target
        assert all(bool(torch.equal(r[j], p[j])) == same[j] for r, p in zip(refs, prefs))
    assert train.plain_frames(btgt, brefs)[0] is btgt and not hasattr(btgt, "_dn_plain")
    hom = train._to_device_batch(raw, cpu, True, True)
    assert hom[2].shape == (4, 4, 4) and torch.equal(train.plain_frames(hom[0], hom[1])[0], btgt)
