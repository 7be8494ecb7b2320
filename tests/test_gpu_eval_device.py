"""The device evaluation chain (csrc/dn_eval.hip, supervised_dispnet_amd/evaluation.py, eval_disp.py --eval-batch) on the GPU: the zoom
against scipy itself, the errors kernel against the fp64 evaluation of kitti_eval.compute_errors, the evaluator against
test_disp.evaluate_sample and the reference's golden numbers, and the command line."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import eval_zoom as Z  # noqa: E402
from supervised_dispnet_amd import _lib, evaluation as EV, kitti_eval as KE  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LO, HI = 1e-3, 80.0
BASE = ["--network", "disp_vgg_BN", "--pretrained-dispnet", "CKPT"]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.int64)


def _device_zoom(planes, targets):
    """planes [B, h, w] float32, targets [(H_b, W_b)] -> (coef [B, h, w] float64, [zoomed + clipped H_b x W_b])."""
    B, h, w = planes.shape
    hw, off, npix, total = EV.ragged_layout(targets)
    d_in = torch.from_numpy(planes).to(DEV)
    coef = torch.empty((B, h, w), dtype=torch.float64, device=DEV)
    out = torch.full((total,), -7.0, dtype=torch.float32, device=DEV)
    d_hw, d_off = torch.from_numpy(hw).to(DEV), torch.from_numpy(off).to(DEV)
    _lib.call("dn_zoom3_prefilter", d_in.data_ptr(), B, h, w, coef.data_ptr(), _stream())
    _lib.call("dn_zoom3_clip", coef.data_ptr(), B, h, w, d_hw.data_ptr(), d_off.data_ptr(), int(hw[:, 0].max()), int(hw[:, 1].max()), LO, HI,
              out.data_ptr(), _stream())
    flat = out.cpu().numpy()
    # nothing is written between the images
    written = np.zeros(total, bool)
    for o, n in zip(off, npix):
        written[o:o + n] = True
    assert np.all(flat[~written] == -7.0)
    return coef.cpu().numpy(), EV.unpack_ragged(flat, hw, off)


# the seven pairs grouped by network resolution (the four KITTI sizes share one batch, in mixed order), then two more for the other code
# paths: a row longer than 1024 (fewer lines per block in the axis-1 prefilter) and a shrinking zoom (coefficients read from global memory)
ZOOM_BATCHES = [((128, 416), [(375, 1242), (370, 1226), (376, 1241), (374, 1238), (370, 1226)]),
                ((256, 352), [(480, 640), (480, 640)]),
                ((192, 640), [(375, 1242)]),
                ((40, 56), [(97, 131), (97, 131), (97, 131)]),
                ((5, 2048), [(9, 2500)]),
                ((40, 56), [(9, 11), (97, 131)])]


@pytest.mark.parametrize("k", range(len(ZOOM_BATCHES)))
def test_zoom_against_scipy(k):
    from scipy.ndimage import spline_filter, zoom
    (h, w), targets = ZOOM_BATCHES[k]
    planes = np.stack([Z.smooth_positive_map(h, w, seed=10 * k + b) for b in range(len(targets))])
    coef, outs = _device_zoom(planes, targets)
    for b, (H, W) in enumerate(targets):
        ref = spline_filter(planes[b], order=3, mode="mirror", output=np.float64)
        assert np.abs(coef[b] - ref).max() <= 1e-12 * np.abs(ref).max()
        want = zoom(planes[b], (H / h, W / w))
        assert want.shape == outs[b].shape == (H, W)
        zero = want == 0
        assert np.all(outs[b][zero] == np.float32(LO))
        if ((h, w), (H, W)) == ((128, 416), (375, 1242)):
            assert zero[374].all()
        if ((h, w), (H, W)) == ((256, 352), (480, 640)):
            assert zero[:, 639].all()
        wb, gb = _bits(want.clip(LO, HI)[~zero]), _bits(outs[b][~zero])
        same = float((wb == gb).mean())
        print("zoom %s -> %s: %.6f %% bit-identical, max ulp %d" % ((h, w), (H, W), 100 * same, np.abs(wb - gb).max()))
        assert np.abs(wb - gb).max() <= 1
        assert same >= 0.999


def _error_images():
    """KITTI density with an odd and an even count, NYU density, an empty mask; offsets deliberately not all 4-aligned."""
    r = np.random.default_rng(5)
    gts, preds, masks = [], [], []
    for (H, W), density, parity in (((375, 1242), 0.0193, 1), ((480, 640), 1.0, None), ((375, 1242), 0.0193, 0), ((8, 9), 0.0, None),
                                    ((37, 53), 0.3, 1)):
        gt = r.uniform(1.0, 79.0, (H, W)).astype(np.float32)
        pred = (gt * r.uniform(0.55, 1.7, (H, W))).astype(np.float32).clip(LO, HI)
        mask = r.random((H, W)) < density
        if parity is not None and int(mask.sum()) % 2 != parity:
            mask[tuple(np.argwhere(mask)[0])] = False
        gts.append(gt), preds.append(pred), masks.append(mask)
    npix = np.array([g.size for g in gts], np.int32)
    off = np.zeros(len(gts), np.int64)
    pos = 0
    for b, n in enumerate(npix):
        off[b] = pos
        pos += int(n) + (3, 1, 2, 4, 0)[b]
    return gts, preds, masks, off, npix, pos


@pytest.fixture(scope="module")
def error_images():
    return _error_images()


@pytest.mark.parametrize("mode", [EV.SCALE_NONE, EV.SCALE_FIXED, EV.SCALE_MEDIAN])
def test_errors_kernel_against_fp64(error_images, mode):
    gts, preds, masks, off, npix, total = error_images
    B = len(gts)
    d = [torch.from_numpy(EV.pack_ragged(a, t, off, total)).to(DEV) for a, t in ((gts, np.float32), (preds, np.float32), (masks, np.uint8))]
    d_off, d_npix = torch.from_numpy(off).to(DEV), torch.from_numpy(npix).to(DEV)
    out = torch.zeros((B, 8), dtype=torch.float32, device=DEV)
    _lib.call("dn_eval_errors", d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_off.data_ptr(), d_npix.data_ptr(), B, mode, 5.4,
              out.data_ptr(), _stream())
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
        ps = p * scale
        assert ps.dtype == np.float32
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


# ---- the evaluator against test_disp.evaluate_sample
def _net():
    import supervised_dispnet_amd.models as models
    from oracle import detgen
    net = models.Disp_vgg_BN(datasets="kitti", with_classifier=False)
    detgen.fill_state_dict(net.state_dict(), "vggbn")
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def net():
    return _net()


def _kitti_samples(n=8, net_hw=(64, 96)):
    """Frames and ~20 %-dense ground truth in four sizes; sample 5 is already at the network's size (it is not resized, so it arrives as
    fp32)."""
    r = np.random.default_rng(11)
    out = []
    for i in range(n):
        H, W = [(120, 180), (118, 176), (121, 181), (119, 178)][i % 4]
        gt = np.where(r.random((H, W)) < 0.2, r.uniform(1, 79, (H, W)), 0.0)
        fh, fw = net_hw if i == 5 else (H, W)
        y, x = np.mgrid[0:fh, 0:fw]
        tgt = np.stack([127 + 100 * np.sin(x / (9.0 + i) + c) * np.cos(y / (7.0 + c)) for c in range(3)], -1) + r.normal(0, 6, (fh, fw, 3))
        out.append({"tgt": tgt.clip(0, 255).astype(np.float32), "gt_depth": gt, "mask": KE.generate_mask(gt, LO, HI)})
    return out


def _nyu_samples(n=8):
    r = np.random.default_rng(12)
    out = []
    for i in range(n):
        H, W = (480, 640) if i == 0 else (120, 160)
        y, x = np.mgrid[0:H, 0:W]
        tgt = np.stack([127 + 100 * np.sin(x / (19.0 + i) + c) * np.cos(y / (17.0 + c)) for c in range(3)]) + r.normal(0, 6, (3, H, W))
        gt = r.uniform(0.0, 10.5, (H, W)).astype(np.float32)
        out.append({"tgt": tgt.clip(0, 255).astype(np.float32), "gt_depth": gt, "mask": KE.generate_nyu_mask(gt, LO, 10)})
    return out


@pytest.mark.parametrize("flags", [[], ["--unsupervised"], ["--stereo"], ["--gt-type", "NYU"]], ids=["supervised", "median", "stereo", "nyu"])
def test_evaluator_against_evaluate_sample(net, flags):
    import eval_disp
    import test_disp
    import supervised_dispnet_amd.utils as U
    nyu = "NYU" in flags
    args = eval_disp.parse_args(BASE + flags + ["--img-height", "64", "--img-width", "96"])
    samples = _nyu_samples() if nyu else _kitti_samples()
    lo, hi = (LO, 10) if nyu else (LO, HI)
    with torch.no_grad():
        host = [test_disp.evaluate_sample(args, net, s, DEV, lo, hi, KE, U) for s in samples]
    n_valid = [int(((s["gt_depth"] > lo) & (s["gt_depth"] < hi)).sum()) if nyu else int(s["mask"].sum()) for s in samples]
    ev = EV.DeviceEvaluator(args, net, DEV, lo, hi, keep_depth=True)
    for bs in (1, 3, 8):
        errs, depths = [], []
        for j0 in range(0, len(samples), bs):
            e, d = ev.evaluate(samples[j0:j0 + bs])
            errs.append(e), depths.extend(d)
        errs = np.concatenate(errs, axis=1)
        assert errs.shape == (7, len(samples)) and errs.dtype == np.float32
        for j, (he, hd) in enumerate(host):
            # the tolerance the eval-mode forward gets against its oracle in this repository (tests/test_gpu_nyu_shapes.py: rtol 1e-3,
            # atol 1e-4 of the largest value): two batch sizes of one forward are held to the same
            np.testing.assert_allclose(depths[j], hd, rtol=1e-3, atol=1e-4 * float(np.abs(hd).max()))
            he = np.asarray(he, np.float64)
            rel = np.abs(errs[:4, j] - he[:4]) / np.abs(he[:4])
            print("batch %d image %d: errors differ by %s, a_k by %s" % (bs, j, rel, np.abs(errs[4:, j] - he[4:]) * n_valid[j]))
            if bs == 1:
                np.testing.assert_allclose(errs[:4, j], he[:4], rtol=1e-5)
                assert np.all(np.abs(errs[4:, j] - he[4:]) <= 1e-5 * he[4:] + 1.0 / n_valid[j])
            else:           # a forward at another batch size: the bound tests/cases.py::check_eval_chain already sets for the errors of
                            # an fp32 network's output (rtol 1e-3, and 3 / n_valid on a_k for pixels within rounding of 1.25^k); the
                            # line printed above shows how many pixels actually flipped (|a_k difference| * n_valid)
                np.testing.assert_allclose(errs[:4, j], he[:4], rtol=1e-3)
                assert np.all(np.abs(errs[4:, j] - he[4:]) <= 1e-3 * he[4:] + 3.0 / n_valid[j])


def test_device_chain_matches_reference_golden(golden, net, tmp_path):
    """The call and tolerance of test_evaluation_chain_matches_reference_golden, through the DeviceEvaluator."""
    import eval_disp
    from cases import check_eval_chain, eval_chain_sample
    g = golden("eval_chain")
    sample = eval_chain_sample(tmp_path)

    def evaluate(flags):
        ev = EV.DeviceEvaluator(eval_disp.parse_args(BASE + flags), net, DEV, 1e-3, 80, keep_depth=True)
        errs, depths = ev.evaluate([sample])
        return errs[:, 0], depths[0]

    check_eval_chain(g, evaluate, rtol=1e-3)


def test_command_line_eval_batch(tmp_path, capsys):
    """eval_disp.main on a synthetic KITTI tree (five frames of one drive, the synthetic velodyne scene of the golden sample): --eval-batch 4
    (a batch of four and a ragged one of one) prints and returns what the per-image chain does, and writes the same-shaped predictions."""
    import shutil
    from PIL import Image
    import eval_disp
    import test_disp
    from cases import eval_chain_sample
    date = tmp_path / "2011_09_26"
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
    (tmp_path / "files.txt").write_text("\n".join(names) + "\n")
    import supervised_dispnet_amd.models as models
    from oracle import detgen
    cli_net = models.DispNetS()                                    # as test_disp.create_disp_net builds it (no 0.5 GB VGG classifier to save)
    detgen.fill_state_dict(cli_net.state_dict(), "dispnets")
    ckpt = tmp_path / "ckpt.pth.tar"
    torch.save({"state_dict": cli_net.state_dict()}, ckpt)
    common = ["--network", "dispnet", "--pretrained-dispnet", str(ckpt), "--dataset-dir", str(tmp_path), "--dataset-list",
              str(tmp_path / "files.txt"), "--unsupervised"]
    want = test_disp.main(common + ["--output-dir", str(tmp_path / "host")])
    host_out = capsys.readouterr().out
    got = eval_disp.main(common + ["--output-dir", str(tmp_path / "dev"), "--eval-batch", "4", "--readers", "2"])
    dev_out = capsys.readouterr().out
    # every printed line but the last (the numbers) is the same text; the last has the same layout
    assert "5 files to test" in dev_out and dev_out.splitlines()[:-1] == host_out.splitlines()[:-1]
    assert len(dev_out.splitlines()[-1]) == len(host_out.splitlines()[-1]) and dev_out.splitlines()[-1].count("&") == 7
    print("means: host %s device %s" % (want, got))
    # batches of four: the bound of the evaluator test for a forward at another batch size (tests/cases.py::check_eval_chain)
    print("a_k: %s pixels differ" % (np.abs(got[4:] - want[4:]) * n_valid))
    np.testing.assert_allclose(got[:4], want[:4], rtol=1e-3)
    assert np.all(np.abs(got[4:] - want[4:]) <= 1e-3 * want[4:] + 3.0 / n_valid)
    ph, pd = np.load(tmp_path / "host" / "predictions.npy"), np.load(tmp_path / "dev" / "predictions.npy")
    assert ph.shape == pd.shape == (5, 128, 416) and ph.dtype == pd.dtype
    np.testing.assert_allclose(pd, ph, rtol=1e-3, atol=1e-4 * float(np.abs(ph).max()))
