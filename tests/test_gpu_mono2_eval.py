"""monodepth2's depth evaluation on the GPU (csrc/dn_eval_mono2.hip, supervised_dispnet_amd/evaluation.py, eval_disp.py --protocol
monodepth2): the three kernels against the fp64 restatement of tests/mono2_eval_audit.py, the evaluator against
the per-image host chain, and the command line."""
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
from supervised_dispnet_amd import _lib, evaluation as EV, kitti_eval as KE  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LO, HI = A.LO, A.HI
NET_HW = (64, 96)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------- post-processing
def _device_post_process(d):
    B, h, w = d.shape[0] // 2, d.shape[1], d.shape[2]
    d_in = torch.from_numpy(d).to(DEV)
    out = torch.full((B, h, w), -7.0, dtype=torch.float32, device=DEV)
    _lib.call("dn_mono2_post_process", d_in.data_ptr(), B, h, w, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", A.PP_SHAPES)
def test_post_process_against_the_restatement(shape):
    B, h, w = shape
    d = np.stack([A.positive_map(h, w, seed=20 + k) for k in range(2 * B)])
    got = _device_post_process(d)
    want = A.post_process(d).astype(np.float32)
    worst = int(A.ulps(got, want).max())
    print("post-process %s: worst distance %d ulp" % (shape, worst))
    assert worst <= 1
    # planes >= B are read mirrored: with them used as they are the left and right borders would come out exchanged
    wrong = A.post_process(np.concatenate([d[:B], d[B:, :, ::-1]])).astype(np.float32)
    assert int(A.ulps(wrong, want).max()) > 1000 and int(A.ulps(got, wrong).max()) > 1000


def test_post_process_takes_the_mirrored_plane_only_at_the_left_border():
    """w = 64: lm = 1 in columns 0 .. 3 (l <= 0.05), rm = 1 in columns 60 .. 63; so there the output IS one of the two inputs."""
    d = np.stack([A.positive_map(8, 64, seed=k) for k in range(4)])
    got = _device_post_process(d)
    assert np.array_equal(got[:, :, :4], d[2:, :, ::-1][:, :, :4]) and np.array_equal(got[:, :, 60:], d[:2, :, 60:])


def test_post_process_refuses_one_column_and_in_place():
    lib = _lib.load()
    t = torch.ones((2, 4, 1), device=DEV)
    o = torch.ones((1, 4, 1), device=DEV)
    assert lib.dn_mono2_post_process(t.data_ptr(), 1, 4, 1, o.data_ptr(), _stream()) != 0 and "dn_mono2_post_process" in _lib.last_error()
    t = torch.ones((2, 4, 8), device=DEV)
    assert lib.dn_mono2_post_process(t.data_ptr(), 1, 4, 8, t.data_ptr(), _stream()) != 0


# ---------------------------------------------------------------------------------------------------------------- resize and invert
def test_resize_recip_against_the_restatement():
    """Every case of one network resolution is one ragged batch (offsets aligned by RAGGED_ALIGN); then all outputs, 1 ulp."""
    for k, ((h, w), targets) in enumerate(A.RESIZE_CASES):
        B = len(targets)
        planes = np.stack([A.positive_map(h, w, seed=40 + 10 * k + b) for b in range(B)])
        hw, off, npix, total = EV.ragged_layout(targets)
        assert np.all(off % EV.RAGGED_ALIGN == 0)
        d_in = torch.from_numpy(planes).to(DEV)
        out = torch.full((total,), -7.0, dtype=torch.float32, device=DEV)
        d_hw, d_off = torch.from_numpy(hw).to(DEV), torch.from_numpy(off).to(DEV)
        _lib.call("dn_bilinear_recip_ragged", d_in.data_ptr(), B, h, w, d_hw.data_ptr(), d_off.data_ptr(), int(hw[:, 0].max()),
                  int(hw[:, 1].max()), out.data_ptr(), _stream())
        torch.cuda.synchronize()
        flat = out.cpu().numpy()
        written = np.zeros(total, bool)
        for o, n in zip(off, npix):
            written[o:o + n] = True
        assert np.all(flat[~written] == -7.0)                           # the gaps between the images stay untouched
        for b, (got, (H, W)) in enumerate(zip(EV.unpack_ragged(flat, hw, off), targets)):
            want = A.resize_recip(planes[b], H, W).astype(np.float32)
            worst = int(A.ulps(got, want).max())
            print("resize %s -> %s: worst distance %d ulp" % ((h, w), (H, W), worst))
            assert got.shape == want.shape and worst <= 1
            if (H, W) == (h, w):
                assert np.array_equal(got, (1.0 / planes[b].astype(np.float64)).astype(np.float32))


def test_resize_recip_into_an_unaligned_image():
    """An image whose offset is no multiple of four elements takes the scalar stores; its neighbours are untouched."""
    (h, w), (H, W) = (8, 16), (11, 37)
    plane = A.positive_map(h, w, seed=3)
    hw = np.array([[H, W]], np.int32)
    off = np.array([3], np.int64)
    out = torch.full((3 + H * W + 5,), -7.0, dtype=torch.float32, device=DEV)
    d_in, d_hw, d_off = torch.from_numpy(plane[None]).to(DEV), torch.from_numpy(hw).to(DEV), torch.from_numpy(off).to(DEV)
    _lib.call("dn_bilinear_recip_ragged", d_in.data_ptr(), 1, h, w, d_hw.data_ptr(), d_off.data_ptr(), H, W, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    flat = out.cpu().numpy()
    assert np.all(flat[:3] == -7.0) and np.all(flat[3 + H * W:] == -7.0)
    assert int(A.ulps(flat[3:3 + H * W].reshape(H, W), A.resize_recip(plane, H, W).astype(np.float32)).max()) <= 1


# ---------------------------------------------------------------------------------------------------------------- errors
@pytest.fixture(scope="module")
def error_images():
    return A.error_images()


@pytest.mark.parametrize("mode", [EV.SCALE_NONE, EV.SCALE_FIXED, EV.SCALE_MEDIAN])
def test_errors_clamp_against_fp64(error_images, mode):
    gts, preds, masks, off, npix, total = error_images
    B = len(gts)
    d = [torch.from_numpy(EV.pack_ragged(a, t, off, total)).to(DEV) for a, t in ((gts, np.float32), (preds, np.float32), (masks, np.uint8))]
    d_off, d_npix = torch.from_numpy(off).to(DEV), torch.from_numpy(npix).to(DEV)
    out = torch.zeros((B, 8), dtype=torch.float32, device=DEV)
    _lib.call("dn_eval_errors_clamp", d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_off.data_ptr(), d_npix.data_ptr(), B, mode, 5.4,
              LO, HI, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    counts = [int(m.sum()) for m in masks]
    assert counts[0] % 2 == 1 and counts[2] % 2 == 0 and 8000 < counts[0] < 10000 and counts[1] == 480 * 640 and counts[3] == 0
    for b in range(B):
        g, p = gts[b][masks[b]], preds[b][masks[b]]
        if counts[b] == 0:
            assert np.all(np.isnan(got[b, :7]))
            assert np.isnan(got[b, 7]) if mode == EV.SCALE_MEDIAN else got[b, 7] == np.float32(1.0 if mode == EV.SCALE_NONE else 5.4)
            continue
        scale = {EV.SCALE_NONE: np.float32(1), EV.SCALE_FIXED: np.float32(5.4), EV.SCALE_MEDIAN: np.median(g) / np.median(p)}[mode]
        assert scale.dtype == np.float32
        raw = p * scale
        ps = raw.clip(np.float32(LO), np.float32(HI))
        assert ps.dtype == np.float32
        n_lo, n_hi = int((raw < np.float32(LO)).sum()), int((raw > np.float32(HI)).sum())
        print("image %d mode %d: %d pixels clamped up to %g, %d down to %g" % (b, mode, n_lo, LO, n_hi, HI))
        if mode != EV.SCALE_NONE:
            assert n_lo > 0 and n_hi > 0
        chain32 = KE.compute_errors(g, ps)
        yard = KE.compute_errors(g.astype(np.float64), ps.astype(np.float64))
        assert got[b, 7].view(np.uint32) == scale.view(np.uint32)
        for k in (4, 5, 6):
            assert got[b, k] == np.float32(chain32[k]), (b, k, got[b, k], chain32[k])
        for k in range(4):
            dist = abs(float(got[b, k]) - yard[k]) / abs(yard[k])
            own = abs(float(chain32[k]) - yard[k]) / abs(yard[k])
            print("image %d mode %d metric %d: device %.3g, numpy float32 %.3g from fp64" % (b, mode, k, dist, own))
            assert dist <= max(own, 2.0 ** -23), (b, k, dist, own)
        want, s = A.errors(gts[b], preds[b], masks[b], mode)
        np.testing.assert_allclose(got[b, :7], want, rtol=2.0 ** -22)
        assert s.view(np.uint32) == got[b, 7].view(np.uint32)


def test_errors_clamp_refuses_bad_bounds():
    lib = _lib.load()
    t = torch.ones(8, device=DEV)
    for lo, hi in ((0.0, 80.0), (2.0, 1.0)):
        assert lib.dn_eval_errors_clamp(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 1, 0, 1.0, lo, hi, t.data_ptr(),
                                        _stream()) != 0
        assert "dn_eval_errors_clamp" in _lib.last_error()


# ---------------------------------------------------------------------------------------------------------------- the evaluator
NET_FLAGS = ["--network", "disp_res_18", "--img-height", str(NET_HW[0]), "--img-width", str(NET_HW[1])]


@pytest.fixture(scope="module")
def weights(tmp_path_factory):
    """A random-weight ResnetEncoder(18) + DepthDecoder saved as a monodepth2 folder (encoder.pth, depth.pth)."""
    import supervised_dispnet_amd.networks as networks
    folder = tmp_path_factory.mktemp("mono2_weights")
    torch.manual_seed(5)
    enc = networks.ResnetEncoder(18, False)
    torch.save(enc.state_dict(), str(folder / "encoder.pth"))
    torch.save(networks.DepthDecoder(enc.num_ch_enc).state_dict(), str(folder / "depth.pth"))
    return str(folder)


@pytest.fixture(scope="module")
def net(weights):
    import eval_disp
    import test_disp
    import supervised_dispnet_amd.models as models
    import supervised_dispnet_amd.networks as networks
    import supervised_dispnet_amd.utils as U
    args = eval_disp.parse_args(NET_FLAGS + ["--pretrained-dispnet", weights, "--mono"])
    return test_disp.create_disp_net(args, models, networks, DEV, U).eval()


@pytest.fixture(scope="module")
def samples():
    return A.kitti_samples(8, NET_HW)


@pytest.mark.parametrize("pp", [False, True], ids=["plain", "post-process"])
@pytest.mark.parametrize("flag", ["--mono", "--stereo"])
def test_evaluator_against_the_host_chain(net, weights, samples, flag, pp):
    import eval_disp
    args = eval_disp.parse_args(NET_FLAGS + ["--pretrained-dispnet", weights, flag, "--protocol", "monodepth2"] + (["--post-process"] if pp else []))
    host = [EV.mono2_evaluate_sample(args, net, s, DEV, LO, HI, pp) for s in samples]
    n_valid = [int(s["mask"].sum()) for s in samples]
    ev = EV.DeviceEvaluator(args, net, DEV, LO, HI, keep_depth=True)
    assert ev.protocol == "monodepth2" and ev.post_process == pp
    for bs in (1, 3, 8):
        errs, depths, scales = [], [], []
        for j0 in range(0, len(samples), bs):
            e, d = ev.evaluate(samples[j0:j0 + bs])
            errs.append(e), depths.extend(d), scales.extend(ev.scales)
        errs = np.concatenate(errs, axis=1)
        assert errs.shape == (7, len(samples)) and errs.dtype == np.float32 and len(scales) == len(samples)
        for j, (he, hs, hd) in enumerate(host):
            assert depths[j].shape == hd.shape == NET_HW
            np.testing.assert_allclose(depths[j], hd, rtol=1e-3, atol=1e-4 * float(np.abs(hd).max()))
            rel = np.abs(errs[:4, j] - he[:4]) / np.abs(he[:4])
            print("%s pp %d batch %d image %d: errors differ by %s, a_k by %s pixels, scale %g / %g" %
                  (flag, pp, bs, j, rel, np.abs(errs[4:, j] - he[4:]) * n_valid[j], scales[j], hs))
            if bs == 1:
                np.testing.assert_allclose(errs[:4, j], he[:4], rtol=1e-5)
                assert np.all(np.abs(errs[4:, j] - he[4:]) <= 1e-5 * he[4:] + 1.0 / n_valid[j])
                np.testing.assert_allclose(scales[j], hs, rtol=1e-5)
            else:           # a forward at another batch size: the bound tests/cases.py::check_eval_chain sets for the errors of an fp32
                            # network's output; the line printed above shows how many pixels actually flipped
                np.testing.assert_allclose(errs[:4, j], he[:4], rtol=1e-3)
                assert np.all(np.abs(errs[4:, j] - he[4:]) <= 1e-3 * he[4:] + 3.0 / n_valid[j])
                np.testing.assert_allclose(scales[j], hs, rtol=1e-3)
        if flag == "--stereo":
            assert np.all(np.asarray(scales) == np.float32(5.4))


def test_the_doubled_forward_keeps_the_first_half(net, weights, samples):
    """Planes 0 .. N-1 of the forward at 2N (frames, then their mirror images) are the forward at N, within the tolerance two batch sizes
    of one forward get; planes N .. 2N-1 of its operand are the frames mirrored exactly."""
    import eval_disp
    args = eval_disp.parse_args(NET_FLAGS + ["--pretrained-dispnet", weights, "--mono", "--protocol", "monodepth2", "--post-process"])
    ev = EV.DeviceEvaluator(args, net, DEV, LO, HI, keep_depth=False)
    img = ev._normalised([EV.prepare_frame(args, s) for s in samples[:3]]).clone()
    both = ev.mirrored(img)
    assert both.shape == (6, 3) + NET_HW and torch.equal(both[:3], img) and torch.equal(both[3:], torch.flip(img, dims=[3]))
    one = ev.forward_disp(img).cpu().numpy()
    two = ev.forward_disp(both).cpu().numpy()
    assert two.shape == (6,) + NET_HW
    np.testing.assert_allclose(two[:3], one, rtol=1e-3, atol=1e-4 * float(np.abs(one).max()))
    assert np.abs(two[3:, :, ::-1] - one).max() > 0                      # the network is not mirror-symmetric: the second half is real work


def test_evaluator_refuses_what_the_protocol_does_not_cover(net, weights):
    import eval_disp
    args = eval_disp.parse_args(NET_FLAGS + ["--pretrained-dispnet", weights, "--mono"])
    with pytest.raises(ValueError, match="--post-process"):
        EV.DeviceEvaluator(args, net, DEV, LO, HI, post_process=True)
    ev = EV.DeviceEvaluator(args, net, DEV, LO, HI, protocol="monodepth2", post_process=True)      # keywords take the place of the flags
    assert ev.protocol == "monodepth2" and ev.post_process


# ---------------------------------------------------------------------------------------------------------------- command line
@pytest.fixture(scope="module")
def kitti_tree(tmp_path_factory, weights):
    """The synthetic KITTI tree of the reference chain's command-line test: five frames of one drive, the synthetic velodyne scene of the
    golden sample.  -> (common argv, valid pixels per frame, directory for outputs)."""
    import shutil
    from PIL import Image
    from cases import eval_chain_sample
    root = tmp_path_factory.mktemp("kitti")
    date = root / "2011_09_26"
    drive = date / "2011_09_26_drive_0002_sync"
    (drive / "image_02" / "data").mkdir(parents=True)
    (drive / "velodyne_points" / "data").mkdir(parents=True)
    n_valid = int(eval_chain_sample(date)["mask"].sum())           # writes the calibration files and 0000000000.bin into `date`
    r = np.random.default_rng(3)
    names = []
    for i in range(5):
        shutil.copy(date / "0000000000.bin", drive / "velodyne_points" / "data" / ("%010d.bin" % i))
        y, x = np.mgrid[0:375, 0:1242]
        img = np.stack([127 + 100 * np.sin(x / (40.0 + 5 * i) + c) * np.cos(y / (30.0 + c)) for c in range(3)], -1) + r.normal(0, 5, (375, 1242, 3))
        Image.fromarray(img.clip(0, 255).astype(np.uint8)).save(drive / "image_02" / "data" / ("%010d.png" % i))
        names.append("2011_09_26/2011_09_26_drive_0002_sync/image_02/data/%010d.png" % i)
    (root / "files.txt").write_text("\n".join(names) + "\n")
    common = ["--network", "disp_res_18", "--pretrained-dispnet", weights, "--dataset-dir", str(root), "--dataset-list", str(root / "files.txt")]
    return common, n_valid, root


RATIOS = " Scaling ratios | med: "


def _numbers_close(got, want, n_valid):
    np.testing.assert_allclose(got[:4], want[:4], rtol=1e-3)
    assert np.all(np.abs(got[4:] - want[4:]) <= 1e-3 * want[4:] + 3.0 / n_valid)


def test_command_line_monodepth2_protocol(kitti_tree, capsys):
    """--eval-batch 4 (a batch of four and a ragged one of one) prints and returns what the per-image host chain (--eval-batch 0) does."""
    import eval_disp
    common, n_valid, root = kitti_tree
    flags = common + ["--mono", "--protocol", "monodepth2", "--post-process"]
    want = eval_disp.main(flags + ["--output-dir", str(root / "host"), "--eval-batch", "0"])
    host_out = capsys.readouterr().out.splitlines()
    got = eval_disp.main(flags + ["--output-dir", str(root / "dev"), "--eval-batch", "4", "--readers", "2"])
    dev_out = capsys.readouterr().out.splitlines()
    print("means: host %s device %s; a_k: %s pixels differ" % (want, got, np.abs(got[4:] - want[4:]) * n_valid))
    assert "5 files to test" in dev_out and len(dev_out) == len(host_out)
    numeric = [i for i, line in enumerate(host_out) if line.startswith(RATIOS) or line.startswith("&")]
    assert len(numeric) == 2 and numeric[1] == len(host_out) - 1 and host_out[numeric[0]].startswith(RATIOS)
    for i, (a, b) in enumerate(zip(dev_out, host_out)):
        if i not in numeric:
            assert a == b
    assert len(dev_out[-1]) == len(host_out[-1]) and dev_out[-1].count("&") == 7
    ratio = lambda line: [float(v) for v in line.replace("|", " ").split() if v[0].isdigit()]      # noqa: E731
    assert dev_out[numeric[0]].startswith(RATIOS) and " | std: " in dev_out[numeric[0]]
    np.testing.assert_allclose(ratio(dev_out[numeric[0]]), ratio(host_out[numeric[0]]), rtol=1e-3, atol=1.5e-3)    # three printed decimals
    _numbers_close(got, want, n_valid)
    ph, pd = np.load(root / "host" / "predictions.npy"), np.load(root / "dev" / "predictions.npy")
    assert ph.shape == pd.shape == (5, 128, 416) and ph.dtype == pd.dtype
    np.testing.assert_allclose(pd, ph, rtol=1e-3, atol=1e-4 * float(np.abs(ph).max()))


def test_command_line_stereo_has_no_ratios_line(kitti_tree, capsys):
    import eval_disp
    common, n_valid, _ = kitti_tree
    flags = common + ["--stereo", "--protocol", "monodepth2"]
    want = eval_disp.main(flags)
    host_out = capsys.readouterr().out
    got = eval_disp.main(flags + ["--eval-batch", "4"])
    dev_out = capsys.readouterr().out
    assert RATIOS not in host_out and RATIOS not in dev_out and dev_out.splitlines()[:-1] == host_out.splitlines()[:-1]
    _numbers_close(got, want, n_valid)


def test_command_line_reference_protocol_is_unchanged(kitti_tree, capsys):
    """--protocol reference is the command without the flag: the same launches on the same inputs, so the same text, and numbers within
    the bound two runs of one forward at one batch size get (rtol 1e-5, one pixel on a_k)."""
    import eval_disp
    common, n_valid, _ = kitti_tree
    flags = common + ["--mono", "--eval-batch", "4"]
    want = eval_disp.main(flags)
    plain_out = capsys.readouterr().out.splitlines()
    got = eval_disp.main(flags + ["--protocol", "reference"])
    flag_out = capsys.readouterr().out.splitlines()
    assert flag_out[:-1] == plain_out[:-1] and not any(line.startswith(RATIOS) for line in flag_out)
    assert len(flag_out[-1]) == len(plain_out[-1]) and flag_out[-1].count("&") == 7
    np.testing.assert_allclose(got[:4], want[:4], rtol=1e-5)
    assert np.all(np.abs(got[4:] - want[4:]) <= 1e-5 * want[4:] + 1.0 / n_valid)
