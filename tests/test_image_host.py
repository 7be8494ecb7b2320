"""Host side of the image chain, no GPU: the numpy restatements of tests/pil_resize.py and the coefficient tables
of supervised_dispnet_amd/inference.py against Pillow and kitti_eval.imresize_bilinear, the contrast and colouring restatements against
PIL and utils.tensor2array, and the command line of run_inference.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import pil_resize as PR  # noqa: E402
from supervised_dispnet_amd import kitti_eval as KE  # noqa: E402

SHAPES = [(375, 1242, 128, 416), (370, 1226, 128, 416), (480, 640, 256, 352), (37, 53, 16, 24), (16, 24, 37, 53), (97, 131, 40, 131),
          (33, 7, 5, 19)]


def _frame(H, W, kind, seed=0):
    r = np.random.RandomState(seed)
    if kind == "full":
        a = r.randint(0, 256, (H, W, 3))
        a.flat[0], a.flat[1] = 0, 255
    elif kind == "low":
        a = r.randint(40, 201, (H, W, 3))
        a.flat[0], a.flat[1] = 40, 200
    else:
        a = np.full((H, W, 3), 77)
    return a.astype(np.uint8)


@pytest.mark.parametrize("H,W,h,w", SHAPES)
def test_resize_restatement_is_pillow(H, W, h, w):
    from PIL import Image
    a = _frame(H, W, "full", seed=H)
    want = np.asarray(Image.fromarray(a).resize((w, h), resample=Image.BILINEAR))
    assert np.array_equal(PR.resize_u8(a, h, w), want)
    # a full-range frame is its own byte-scale, so the whole chain is the same picture
    assert np.array_equal(PR.imresize(a.astype(np.float32), h, w), KE.imresize_bilinear(a.astype(np.float32), (h, w)))


@pytest.mark.parametrize("kind", ["low", "constant"])
@pytest.mark.parametrize("H,W,h,w", [(37, 53, 16, 24), (33, 90, 16, 24), (370, 1226, 128, 416)])
def test_bytescale_restatement(kind, H, W, h, w):
    a = _frame(H, W, kind, seed=W).astype(np.float32)
    want = KE.imresize_bilinear(a, (h, w))
    assert np.array_equal(PR.imresize(a, h, w), want)
    if kind == "constant":
        assert not want.any()
    else:
        assert not np.array_equal(want, PR.resize_u8(a.astype(np.uint8), h, w))          # stretched before the resize


@pytest.mark.parametrize("H,W,h,w", SHAPES)
def test_coefficient_tables_match_the_restatement(H, W, h, w):
    from supervised_dispnet_amd import inference
    for n, O in ((W, w), (H, h)):
        first, count, k = inference.resize_coefficients(n, O)
        rows = PR.coefficients(n, O)
        assert k.shape == (O, max(len(r[1]) for r in rows))
        for o, (f, kk) in enumerate(rows):
            assert first[o] == f and count[o] == len(kk)
            assert np.array_equal(k[o, :len(kk)], kk) and not k[o, len(kk):].any()
        t = inference.table_rows(n, O)
        assert t.dtype == np.int32 and t.shape == (O, 2 + k.shape[1])
    assert inference.resize_coefficients(1242, 416)[2].shape[1] == 6 and inference.resize_coefficients(33, 5)[2].shape[1] == 14


def test_contrast_restatement_is_pil():
    from PIL import Image, ImageEnhance
    r = np.random.RandomState(1)
    for kind in ("random", "low", "constant"):
        im = r.randint(0, 256, (20, 30, 3)).astype(np.uint8)
        if kind == "low":
            im = (im // 4 + 100).astype(np.uint8)
        if kind == "constant":
            im[:] = 77
        for factor in (4.0, 0.5):
            want = np.asarray(ImageEnhance.Contrast(Image.fromarray(im)).enhance(factor))
            assert np.array_equal(PR.contrast(im, factor), want), (kind, factor)


def test_colorize_restatement_is_tensor2array():
    import supervised_dispnet_amd.utils as U
    r = np.random.RandomState(2)
    table = r.randint(0, 256, (256, 3)).astype(np.uint8)
    x = r.uniform(0.0, 12.0, (19, 45)).astype(np.float32)
    for max_value in (None, 10):
        for tab in (table, None):
            if tab is None and U.colour_table("bone") is not None:
                continue                                          # with OpenCV tensor2array has no grey branch to compare with
            arr = U.tensor2array(torch.from_numpy(x.copy())[None], max_value=max_value, colormap="bone", channel_first=False, table=tab)
            assert arr.dtype == np.float32 and arr.shape == (19, 45, 3)
            assert np.array_equal(PR.colorize(x, max_value, tab), (255 * arr).astype(np.uint8))
    # channel_first and the 2-D form; the [3, h, w] branch
    a2 = U.tensor2array(torch.from_numpy(x.copy()), max_value=10, table=table)
    assert a2.shape == (3, 19, 45) and np.array_equal((255 * a2).astype(np.uint8).transpose(1, 2, 0), PR.colorize(x, 10, table))
    rgb = torch.from_numpy(r.uniform(-1, 1, (3, 4, 5)).astype(np.float32))
    assert np.array_equal(U.tensor2array(rgb, channel_first=False), (0.5 + rgb.numpy() * 0.5).transpose(1, 2, 0))
    # the table's bytes are the output's bytes: /255 and 255* is the identity on all 256 values
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal((255 * (v.astype(np.float32) / 255)).astype(np.uint8), v)


def test_frames_are_refused_by_name():
    from supervised_dispnet_amd import inference
    for bad in (np.zeros((4, 5), np.uint8), np.zeros((4, 5, 4), np.uint8), np.zeros((4, 5, 3), np.float32)):
        with pytest.raises(ValueError, match="a/b.png.*H x W x 3 uint8"):
            inference.check_frame(bad, "a/b.png")
    assert inference.garg_rectangle(128, 416) == (52, 126, 14, 401)


def test_run_inference_help_lists_the_reference_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "run_inference.py"), "--help"], stdout=subprocess.PIPE, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--network", "--imagenet-normalization", "--monodepth2", "--output-disp", "--output-depth", "--pretrained", "--img-height",
                 "--img-width", "--no-resize", "--dataset-list", "--dataset-dir", "--output-dir", "--img-exts", "--batch", "--readers",
                 "--host-chain"):
        assert flag in out.stdout, flag
    from supervised_dispnet_amd import inference
    d = inference.build_parser().parse_args(["--pretrained", "x"])
    assert (d.network, d.img_height, d.img_width, d.dataset_dir, d.output_dir, d.img_exts, d.batch) == \
        ("disp_vgg", 128, 416, ".", "output", ["png", "jpg", "bmp"], 8)
