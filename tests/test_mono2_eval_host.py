"""monodepth2's depth evaluation without a GPU: the fp64 restatement of tests/mono2_eval_audit.py against torch's
own bilinear resize and against closed forms, the host chain of supervised_dispnet_amd.evaluation against the restatement, and
eval_disp.py's new flags."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import mono2_eval_audit as A  # noqa: E402
from supervised_dispnet_amd import evaluation as EV  # noqa: E402

BASE = ["--network", "disp_res_18", "--pretrained-dispnet", "FOLDER"]
RESIZES = [(hw, t) for hw, targets in A.RESIZE_CASES for t in targets]


@pytest.mark.parametrize("hw,target", RESIZES)
def test_restated_resize_is_torch_bilinear(hw, target):
    import torch.nn.functional as F
    d = A.positive_map(hw[0], hw[1], seed=3)
    want = F.interpolate(torch.from_numpy(d).double()[None, None], size=target, mode="bilinear", align_corners=False)[0, 0].numpy()
    got = A.resize(d, *target)
    worst = float((np.abs(got - want) / np.abs(want)).max())
    print("resize %s -> %s: worst relative difference from torch %.3g" % (hw, target, worst))
    assert got.shape == tuple(target) and worst <= 1e-12


def test_equal_sizes_return_the_input_exactly():
    d = A.positive_map(6, 10, seed=4)
    assert np.array_equal(A.resize(d, 6, 10), d.astype(np.float64))
    assert np.array_equal(EV.mono2_resize_recip(d, (6, 10)), (1.0 / d.astype(np.float64)).astype(np.float32))


def test_post_process_closed_forms():
    lm = A.left_ramp(21)
    assert lm[0] == 1.0 and lm[1] == 1.0 and np.all(lm[2:] == 0.0)         # x = 1: l = 0.05 exactly; x = 2: 20 (0.1 - 0.05) = 1
    lm = A.left_ramp(20)
    assert lm[0] == 1.0 and lm[1] == 1.0 - 20.0 * (1.0 / 19.0 - 0.05) and 0.94 < lm[1] < 0.95 and np.all(lm[2:] == 0.0)
    for w in list(range(2, 70)) + [416, 640, 1024]:
        lm = A.left_ramp(w)
        assert np.all(lm * lm[::-1] == 0.0), w                               # the two ramps never overlap
        a, b = EV.mono2_ramps(w)
        assert np.array_equal(a, lm) and np.array_equal(b, lm[::-1])
    const = np.full((2, 5, 37), np.float32(0.7))
    assert np.all(A.post_process(const).astype(np.float32) == np.float32(0.7))
    L = A.positive_map(5, 37, seed=9)
    both = np.stack([L, L[:, ::-1]])                                         # the second prediction, un-mirrored, equals the first
    assert np.all(A.ulps(A.post_process(both)[0].astype(np.float32), L) <= 1)
    assert np.all(A.ulps(EV.mono2_post_process(L, L[:, ::-1]), L) <= 1)


@pytest.mark.parametrize("shape", A.PP_SHAPES)
def test_host_post_process_equals_the_restatement(shape):
    B, h, w = shape
    d = np.stack([A.positive_map(h, w, seed=20 + k) for k in range(2 * B)])
    want = A.post_process(d).astype(np.float32)
    for b in range(B):
        assert np.array_equal(EV.mono2_post_process(d[b], d[B + b]), want[b])


@pytest.mark.parametrize("hw,target", RESIZES)
def test_host_resize_equals_the_restatement(hw, target):
    d = A.positive_map(hw[0], hw[1], seed=5)
    got = EV.mono2_resize_recip(d, target)
    assert got.dtype == np.float32 and np.all(A.ulps(got, A.resize_recip(d, *target).astype(np.float32)) <= 1)


def test_clamp_after_scale_differs_from_clip_before_scale():
    from supervised_dispnet_amd import kitti_eval as KE
    gt, pred, mask = A.clamp_case()
    want, s = A.errors(gt, pred, mask, A.SCALE_MEDIAN)
    scaled = pred[mask] * s
    n_above = int((scaled > 80).sum())
    print("median ratio %.3f, %d of %d pixels end above 80" % (s, n_above, scaled.size))
    assert 2.0 < s < 2.6 and 50 < n_above < 400
    before = pred.clip(A.LO, A.HI)[mask]                                    # the reference's order: clip, then scale, no clamp
    ref = KE.compute_errors(gt[mask], before * (np.median(gt[mask]) / np.median(before)))
    got, gs = EV.mono2_errors(gt, pred, mask, EV.SCALE_MEDIAN, 1.0, A.LO, A.HI)
    print("abs_rel: clamp after the scale %.4f, clip before it %.4f" % (got[0], ref[0]))
    assert gs.dtype == np.float32 and gs == s
    np.testing.assert_allclose(got, want, rtol=1e-12)
    assert abs(got[0] - ref[0]) > 1e-3 * ref[0] and got[0] < ref[0]
    assert float(np.minimum(scaled, 80).max()) == 80.0


@pytest.mark.parametrize("mode", [EV.SCALE_NONE, EV.SCALE_FIXED, EV.SCALE_MEDIAN])
def test_host_errors_equal_the_restatement(mode):
    gts, preds, masks, _, _, _ = A.error_images()
    assert (EV.SCALE_NONE, EV.SCALE_FIXED, EV.SCALE_MEDIAN) == (A.SCALE_NONE, A.SCALE_FIXED, A.SCALE_MEDIAN) and EV.STEREO_SCALE == A.STEREO_SCALE
    for b in (0, 2, 3, 4):                                                   # (the 480 x 640 image is the GPU test's)
        want, s = A.errors(gts[b], preds[b], masks[b], mode)
        got, gs = EV.mono2_errors(gts[b], preds[b], masks[b], mode, EV.STEREO_SCALE, A.LO, A.HI)
        if not masks[b].any():
            assert np.all(np.isnan(got)) and np.all(np.isnan(want))
            assert np.isnan(gs) if mode == EV.SCALE_MEDIAN else gs == s
            continue
        assert gs.view(np.uint32) == s.view(np.uint32)
        np.testing.assert_allclose(got[:4], want[:4], rtol=1e-12)
        assert np.array_equal(got[4:], want[4:])


@pytest.mark.parametrize("pp", [False, True])
def test_host_chain_equals_the_restatement(pp):
    r = np.random.default_rng(2)
    gt = np.where(r.random((37, 53)) < 0.4, r.uniform(1, 79, (37, 53)), 0.0)
    mask = (gt > A.LO) & (gt < A.HI)
    d, dm = A.positive_map(12, 20, seed=1), A.positive_map(12, 20, seed=2)
    for mode in (EV.SCALE_NONE, EV.SCALE_FIXED, EV.SCALE_MEDIAN):
        want, s = A.chain(d, dm if pp else None, gt, mask, mode)
        got, gs, used = EV.mono2_host_chain(d, dm if pp else None, gt, mask, mode, EV.STEREO_SCALE, A.LO, A.HI)
        assert used.shape == d.shape and (pp or np.array_equal(used, d))
        np.testing.assert_allclose(gs, s, rtol=2e-7)
        np.testing.assert_allclose(got[:4], want[:4], rtol=1e-5)
        assert np.all(np.abs(got[4:] - want[4:]) <= 1.0 / mask.sum())


def test_parser_defaults_and_refusals():
    import eval_disp
    args = eval_disp.parse_args(BASE)
    assert args.protocol == "reference" and args.post_process is False
    args = eval_disp.parse_args(BASE + ["--mono", "--protocol", "monodepth2", "--post-process", "--eval-batch", "4"])
    assert args.protocol == "monodepth2" and args.post_process and args.eval_batch == 4
    assert eval_disp.parse_args(BASE + ["--stereo", "--protocol", "monodepth2"]).post_process is False
    for flags, named in ((["--post-process"], "--post-process"),
                         (["--protocol", "reference", "--post-process"], "--post-process"),
                         (["--protocol", "monodepth2", "--gt-type", "NYU"], "--gt-type NYU"),
                         (["--protocol", "monodepth2", "--network", "DORN"], "--network DORN"),
                         (["--protocol", "monodepth2", "--network", "disp_vgg_BN_DORN"], "--network disp_vgg_BN_DORN"),
                         (["--protocol", "monodepth2", "--error"], "--error")):
        with pytest.raises(SystemExit) as e:
            eval_disp.parse_args(BASE + flags)
        assert named in str(e.value) and "\n" not in str(e.value), (flags, str(e.value))
    with pytest.raises(SystemExit):
        eval_disp.parse_args(BASE + ["--protocol", "cv2"])


def test_new_flags_are_not_handed_to_the_reference_command_line():
    import eval_disp
    argv = BASE + ["--protocol", "reference", "--mono", "--post-process", "--eval-batch", "0"]
    assert eval_disp.host_chain_argv(argv) == BASE + ["--mono"]


def test_reference_protocol_without_eval_batch_is_still_the_host_chain(monkeypatch):
    import eval_disp
    import test_disp
    seen = []
    monkeypatch.setattr(test_disp, "main", lambda argv: seen.append(argv) or "host")
    assert eval_disp.main(BASE + ["--protocol", "reference"]) == "host" and seen == [BASE]
