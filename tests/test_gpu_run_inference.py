"""run_inference.py and eval_disp.py --device-resize on the GPU: the device chain writes the files of the
reference's per-image host chain (--host-chain), pixel for pixel."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from supervised_dispnet_amd import inference  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [(47, 150), (50, 160)]
NET_HW = ["--img-height", "32", "--img-width", "96"]


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """A freshly initialised disp_vgg_BN saved as run_inference.py loads it, and six PNG frames of two sizes."""
    from PIL import Image
    import supervised_dispnet_amd.models as models
    root = tmp_path_factory.mktemp("inference")
    torch.manual_seed(0)
    ckpt = root / "dispnet_checkpoint.pth.tar"
    torch.save({"state_dict": models.Disp_vgg_BN().state_dict()}, ckpt)
    frames = root / "frames"
    frames.mkdir()
    r = np.random.RandomState(4)
    for i in range(6):
        H, W = SIZES[i % 2]
        y, x = np.mgrid[0:H, 0:W]
        img = np.stack([120 + 90 * np.sin(x / (7.0 + i) + c) * np.cos(y / (5.0 + c)) for c in range(3)], -1) + r.normal(0, 5, (H, W, 3))
        Image.fromarray(img.clip(0, 255).astype(np.uint8)).save(frames / ("%06d.png" % (10 * i)))
    return root, ["--network", "disp_vgg_BN", "--pretrained", str(ckpt), "--dataset-dir", str(frames), "--output-disp", "--output-depth"] + NET_HW


def _run(scene, name, extra, **kw):
    import run_inference
    root, common = scene
    res = run_inference.main(common + ["--output-dir", str(root / name)] + extra, keep_outputs=True, **kw)
    assert sorted(os.listdir(res["output_dir"])) == sorted(res["files"])
    return res


def _read(res, name):
    from PIL import Image
    return np.asarray(Image.open(os.path.join(res["output_dir"], name)))


NAMES = sorted(["%d_%s.png" % (j, k) for j in range(6) for k in ("disp", "en")] + ["%06d_depth.png" % (10 * j) for j in range(6)])


def test_device_chain_writes_the_host_chain_files(scene):
    host = _run(scene, "host", ["--host-chain"])
    dev = _run(scene, "dev1", ["--batch", "1", "--readers", "2"])
    assert sorted(host["files"]) == sorted(dev["files"]) == NAMES
    r0, r1, c0, c1 = inference.garg_rectangle(32, 96)
    for name in NAMES:
        a, b = _read(host, name), _read(dev, name)
        assert a.shape == b.shape == ((32, 96, 3) if name.endswith("_depth.png") else (r1 - r0, c1 - c0, 3)) and a.dtype == np.uint8
        assert np.array_equal(a, b), name
    for a, b in zip(host["outputs"], dev["outputs"]):                    # the same input bits at the same batch size: the same forward
        assert np.array_equal(a, b)
    assert len({_read(dev, n).tobytes() for n in NAMES if n.endswith("_disp.png")}) == 6      # six pictures, not one


@pytest.mark.parametrize("tables", ["opencv-or-grey", "explicit"])
def test_batched_device_chain(scene, tables):
    """--batch 4 (a batch of four of both frame sizes and one of two): every file is the host post-processing of the network output the
    batch gave."""
    r = np.random.RandomState(5)
    tabs = None if tables != "explicit" else {k: r.randint(0, 256, (256, 3)).astype(np.uint8) for k in ("bone", "rainbow")}
    res = _run(scene, "dev4-" + tables, ["--batch", "4"], tables=tabs)
    assert sorted(res["files"]) == NAMES and len(res["outputs"]) == 6
    args = inference.build_parser().parse_args(scene[1])
    import supervised_dispnet_amd.utils as U
    host_tabs = tabs if tabs is not None else {k: U.colour_table(k) for k in ("bone", "rainbow")}
    for j, out in enumerate(res["outputs"]):
        assert out.shape == (32, 96) and out.dtype == np.float32
        want = inference.host_images(args, torch.from_numpy(out)[None], host_tabs)
        for kind, name in (("disp", "%d_disp.png" % j), ("en", "%d_en.png" % j), ("depth", "%06d_depth.png" % (10 * j))):
            assert np.array_equal(_read(res, name), want[kind]), name
    if tabs is not None:                                                # the table's bytes are the picture's bytes
        assert set(map(tuple, _read(res, "0_disp.png").reshape(-1, 3))) <= set(map(tuple, tabs["bone"]))


def test_no_resize_needs_one_size_per_batch(scene):
    with pytest.raises(ValueError, match="frames of one size per batch"):
        _run(scene, "mixed", ["--batch", "4", "--no-resize"])


def test_eval_disp_device_resize_prints_the_same_lines(tmp_path, capsys):
    """eval_disp.main --eval-batch 4 on the synthetic KITTI tree of tests/test_gpu_eval_device.py (five 375 x 1242 frames, one already at
    the network's size would not be KITTI): with --device-resize the network sees the same bits, so every printed line is the same."""
    import shutil
    from PIL import Image
    import eval_disp
    from cases import eval_chain_sample
    import supervised_dispnet_amd.models as models
    from oracle import detgen
    date = tmp_path / "2011_09_26"
    drive = date / "2011_09_26_drive_0002_sync"
    (drive / "image_02" / "data").mkdir(parents=True)
    (drive / "velodyne_points" / "data").mkdir(parents=True)
    eval_chain_sample(date)                                             # writes the calibration files and 0000000000.bin into `date`
    r = np.random.default_rng(3)
    names = []
    for i in range(5):
        shutil.copy(date / "0000000000.bin", drive / "velodyne_points" / "data" / ("%010d.bin" % i))
        y, x = np.mgrid[0:375, 0:1242]
        img = np.stack([127 + 100 * np.sin(x / (40.0 + 5 * i) + c) * np.cos(y / (30.0 + c)) for c in range(3)], -1) + r.normal(0, 5, (375, 1242, 3))
        Image.fromarray(img.clip(0, 255).astype(np.uint8)).save(drive / "image_02" / "data" / ("%010d.png" % i))
        names.append("2011_09_26/2011_09_26_drive_0002_sync/image_02/data/%010d.png" % i)
    (tmp_path / "files.txt").write_text("\n".join(names) + "\n")
    net = models.DispNetS()
    detgen.fill_state_dict(net.state_dict(), "dispnets")
    ckpt = tmp_path / "ckpt.pth.tar"
    torch.save({"state_dict": net.state_dict()}, ckpt)
    common = ["--network", "dispnet", "--pretrained-dispnet", str(ckpt), "--dataset-dir", str(tmp_path), "--dataset-list",
              str(tmp_path / "files.txt"), "--unsupervised", "--eval-batch", "4", "--readers", "2"]
    want = eval_disp.main(common + ["--output-dir", str(tmp_path / "host")])
    host_out = capsys.readouterr().out
    got = eval_disp.main(common + ["--output-dir", str(tmp_path / "dev"), "--device-resize"])
    dev_out = capsys.readouterr().out
    assert "5 files to test" in dev_out and dev_out == host_out
    assert np.array_equal(got, want)
    assert np.array_equal(np.load(tmp_path / "host" / "predictions.npy"), np.load(tmp_path / "dev" / "predictions.npy"))
    with pytest.raises(SystemExit, match="--eval-batch"):
        eval_disp.parse_args(common[:-4] + ["--device-resize"])
