"""Host side of prepare_train_data.py, no GPU: the numpy restatement of the velodyne depth map
(tests/velo_depth.py) and the restated KittiRawLoader against what the REFERENCE's loader produced on the fabricated tree
(tests/golden/kitti_prep.npz) and against tests/golden/kitti_gt.npz; the resize without the byte-scale against PIL;
prepare_train_data.py --host-chain end to end, its dump read by the project's folder readers and by tools/make_shards.py."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import kitti_raw_tree as T  # noqa: E402
import pil_resize as PR  # noqa: E402
import velo_depth as VD  # noqa: E402
from cases import _golden_generator  # noqa: E402
from supervised_dispnet_amd import kitti_prep as KP  # noqa: E402

H, W = 16, 48


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    base = tmp_path_factory.mktemp("kitti_raw")
    return {"root": T.write_tree(base / "raw"), "static": T.write_static_frames(base / "static.txt"),
            "held": T.write_test_scenes(base / "test_scenes.txt"), "base": base}


def _dense(g, key, shape):
    d = np.zeros(shape, np.float32)
    yx = g[key + ":yx"].astype(np.int64)
    d[yx[:, 0], yx[:, 1]] = g[key + ":val"]
    return d


@pytest.mark.parametrize("mode", ["speed", "static"])
@pytest.mark.parametrize("ratio", [1, 2])
def test_loader_and_restatement_match_the_reference(tree, golden, mode, ratio):
    g = golden("kitti_prep")
    loader = KP.KittiRawLoader(tree["root"], static_frames_file=tree["static"] if mode == "static" else None, img_height=H, img_width=W,
                               get_depth=True, get_pose=True, depth_size_ratio=ratio, test_scenes=T.HELD_OUT)
    run = "%s:r%d" % (mode, ratio)
    scenes = [s for drive in loader.scenes for s in loader.collect_scenes(drive)]
    assert [s["rel_path"] for s in scenes] == list(g[run + ":scenes"])
    shape, lims = loader.depth_shape()
    assert shape == (H // ratio, W // ratio)
    maps = 0
    for scene in scenes:
        key = run + ":" + scene["rel_path"]
        picked = loader.frames(scene)
        np.testing.assert_array_equal(np.array([int(f) for _, f in picked]), g[key + ":ids"])
        np.testing.assert_array_equal(scene["P_rect"], g[key + ":P_rect"])
        np.testing.assert_array_equal(scene["intrinsics"], g[key + ":intrinsics"])
        poses = np.array([scene["pose"][i] for i, _ in picked]).reshape(-1, 12)
        np.testing.assert_allclose(poses, g[key + ":poses"], rtol=1e-6, atol=1e-9)
        M = loader.velo2im(scene)
        for i, frame_id in picked:
            cloud = KP.read_cloud(loader.velo_file(scene, i))
            want = _dense(g, "%s:depth:%s" % (key, frame_id), shape)
            np.testing.assert_array_equal(VD.depth_map(cloud, M, shape[0], shape[1], *lims), want)
            np.testing.assert_array_equal(loader.host_depth_map(scene, cloud), want)
            maps += 1
    assert maps >= 9


@pytest.mark.parametrize("shape", [(375, 1242), (120, 400)])
def test_restatement_equals_kitti_gt_golden_in_fp32(golden, shape):
    g = golden("kitti_gt")
    cloud, M = VD.kitti_gt_inputs(_golden_generator())
    want = VD.golden_map(g, shape)
    got = VD.depth_map(cloud, M, shape[0], shape[1])
    print("%dx%d: %d pixels differ" % (shape[0], shape[1], int((got != want).sum())))
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("case", [(40, 120, 16, 48), (375, 1242, 128, 416), (16, 48, 16, 48)])
def test_resize_without_stretch_equals_pil(case):
    from PIL import Image
    H0, W0, h, w = case
    frame = T.frame("2011_09_26", "0801", "02", 3, H0, W0)
    assert frame.min() > 0 and frame.max() < 255                     # a byte-scale would change it
    want = np.asarray(Image.fromarray(frame).resize((w, h), Image.BILINEAR))
    np.testing.assert_array_equal(PR.resize_u8(frame, h, w), want)
    np.testing.assert_array_equal(KP.host_resize(frame, h, w), want)
    if (H0, W0) == (h, w):
        np.testing.assert_array_equal(want, frame)


def _dump(tree, name, extra=()):
    import prepare_train_data
    out = str(tree["base"] / name)
    res = prepare_train_data.main([tree["root"], "--dump-root", out, "--height", str(H), "--width", str(W), "--with-depth", "--with-pose",
                                   "--host-chain", "--test-scenes", tree["held"], "--readers", "2"] + list(extra))
    return out, res


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, n), root) for d, _, names in os.walk(root) for n in names)


def test_host_chain_dump(tree):
    from PIL import Image
    out, res = _dump(tree, "dump_speed")
    loader = KP.KittiRawLoader(tree["root"], img_height=H, img_width=W, get_depth=True, get_pose=True, test_scenes=T.HELD_OUT)
    want_files = ["train.txt", "val.txt"]
    kept = []
    for drive in loader.scenes:
        for scene in loader.collect_scenes(drive):
            picked = loader.frames(scene)
            if len(picked) < 3:
                continue                                              # drive 0802: one frame, its folders are removed
            kept.append(scene["rel_path"])
            folder = os.path.join(out, scene["rel_path"])
            want_files += [os.path.join(scene["rel_path"], n) for n in ["cam.txt", "poses.txt"]]
            np.testing.assert_array_equal(np.genfromtxt(os.path.join(folder, "cam.txt")), scene["intrinsics"])
            text = open(os.path.join(folder, "poses.txt")).read().split("\n")
            assert text[:-1] == [" ".join("%.6e" % v for v in scene["pose"][i].reshape(-1)) for i, _ in picked] and text[-1] == ""
            M = loader.velo2im(scene)
            for i, frame_id in picked:
                want_files += [os.path.join(scene["rel_path"], frame_id + ext) for ext in (".jpg", ".npy")]
                depth = np.load(os.path.join(folder, frame_id + ".npy"))
                assert depth.dtype == np.float32
                np.testing.assert_array_equal(depth, VD.depth_map(KP.read_cloud(loader.velo_file(scene, i)), M, H, W))
                buf = io.BytesIO()
                Image.fromarray(PR.resize_u8(KP.read_frame(loader.image_file(scene, i)), H, W)).save(buf, format="JPEG")
                assert open(os.path.join(folder, frame_id + ".jpg"), "rb").read() == buf.getvalue()
    assert len(kept) == 4 and sorted(res["scenes"]) == sorted(kept)
    assert _files(out) == sorted(want_files)
    # the split: sorted prefixes, one draw each under seed 8964, both cameras of a drive on the same side
    np.random.seed(8964)
    train, val = [], []
    for pr in sorted(set(k[:-2] for k in kept)):
        (val if np.random.random() < 0.1 else train).extend(sorted(k for k in kept if k.startswith(pr)))
    assert open(os.path.join(out, "train.txt")).read().split() == train and open(os.path.join(out, "val.txt")).read().split() == val
    assert train


def test_dump_feeds_the_folder_readers_and_make_shards(tree):
    from supervised_dispnet_amd import data as D
    out, _ = _dump(tree, "dump_static", ["--static-frames", tree["static"]])
    assert len([n for n in os.listdir(out) if n.endswith(("_02", "_03"))]) == 6        # every folder keeps 6 frames
    ds = D.SequenceFolder(out, seed=0, train=True, transform=D.Transform(*D.normalization(), flip=False))
    img, gt = ds[0]
    assert tuple(img.shape) == (3, H, W) and tuple(gt.shape) == (H, W) and float(gt.max()) > 0
    shards = str(tree["base"] / "shards")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_shards.py"), out, shards], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    assert "%dx%d" % (H, W) in p.stdout and os.path.isfile(os.path.join(shards, "meta.json"))


def test_no_train_gt_and_ratio(tree):
    out, _ = _dump(tree, "dump_r2", ["--depth-size-ratio", "2", "--no-train-gt"])
    train = open(os.path.join(out, "train.txt")).read().split()
    val = open(os.path.join(out, "val.txt")).read().split()
    for s in train:
        assert not [n for n in os.listdir(os.path.join(out, s)) if n.endswith(".npy")]
    for s in val:
        assert np.load(os.path.join(out, s, sorted(n for n in os.listdir(os.path.join(out, s)) if n.endswith(".npy"))[0])).shape == (8, 24)


def test_refused_cases(tree, capsys):
    import prepare_train_data
    with pytest.raises(SystemExit, match="cityscapes is not implemented"):
        prepare_train_data.main([tree["root"], "--dataset-format", "cityscapes", "--host-chain"])
    with pytest.raises(SystemExit, match="multiples of --depth-size-ratio"):
        prepare_train_data.main([tree["root"], "--host-chain", "--height", "16", "--width", "50", "--depth-size-ratio", "4"])
    out = str(tree["base"] / "dump_all")
    prepare_train_data.main([tree["root"], "--dump-root", out, "--height", str(H), "--width", str(W), "--host-chain"])
    assert "no drive is held out" in capsys.readouterr().err
    assert os.path.isdir(os.path.join(out, "2011_09_28_drive_0002_sync_02"))
    assert not [n for n in os.listdir(os.path.join(out, "2011_09_28_drive_0002_sync_02")) if n.endswith((".npy", "poses.txt"))]
