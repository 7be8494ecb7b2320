"""prepare_train_data.py on the GPU: dn_velo_depth against hand-made cases, against tests/velo_depth.py and
against tests/golden/kitti_gt.npz, dn_resize_u8 against PIL, and the device chain of the command against its --host-chain -- every
pixel, byte and file equal."""
import itertools
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

import kitti_raw_tree as T  # noqa: E402
import velo_depth as VD  # noqa: E402
from cases import _golden_generator  # noqa: E402
from supervised_dispnet_amd import _lib, inference, kitti_eval as KE, kitti_prep as KP  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
h, w = 6, 5
EYE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float64)
NEG = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, -4]], dtype=np.float64)      # depth = x - 4: negative for 0 <= x < 4


@pytest.fixture(scope="module")
def ops():
    return inference.ImageOps(DEV)


def P(r, c, z):
    """A point that EYE puts on pixel (r, c) with depth z: u = c + 1 and v = r + 1 exactly for dyadic z."""
    return [(c + 1) * z, (r + 1) * z, z, 0.5]


def N(r, c, x):
    """A point that NEG puts on pixel (r, c) with depth x - 4."""
    return [x, (c + 1) * (x - 4), (r + 1) * (x - 4), 0.5]


def run(ops, clouds, Ms, shape=(h, w), lims=None):
    clouds = [np.asarray(c, dtype=np.float32).reshape(-1, 4) for c in clouds]
    _, depth = KP.device_batch(ops, None, None, clouds, np.stack(Ms), shape, lims or shape)
    return depth


def expect(hits, shape=(h, w)):
    out = np.zeros(shape, np.float32)
    for (r, c), v in hits.items():
        out[r, c] = v
    return out


def test_hand_made_cases(ops):
    nan, inf = float("nan"), float("inf")
    cases = []
    # three points on one pixel, in each order: the minimum wins
    for order in itertools.permutations([4.0, 2.0, 8.0]):
        cases.append((EYE, [P(2, 3, z) for z in order], {(2, 3): 2.0}))
    # (r, 0) and (r - 1, w - 1) share a key: the minimum goes to the FIRST point's pixel, the other keeps its own last write
    cases.append((EYE, [P(3, 0, 8.0), P(2, 4, 4.0)], {(3, 0): 4.0, (2, 4): 4.0}))
    cases.append((EYE, [P(2, 4, 4.0), P(3, 0, 8.0)], {(2, 4): 4.0, (3, 0): 8.0}))
    cases.append((EYE, [P(2, 4, 8.0), P(3, 0, 4.0)], {(2, 4): 4.0, (3, 0): 4.0}))
    cases.append((EYE, [P(3, 0, 4.0), P(2, 4, 8.0), P(2, 4, 16.0)], {(3, 0): 4.0, (2, 4): 16.0}))
    # u = 2.5 and 3.5 round to 2 and 4: columns 1 and 3
    cases.append((EYE, [[5.0, 4.0, 2.0, 0], [14.0, 8.0, 4.0, 0]], {(1, 1): 2.0, (1, 3): 4.0}))
    # col = -1 (u = 0), col = lim_w (u = 6), row = lim_h (v = 7): dropped; the corners are kept
    cases.append((EYE, [[0.0, 2.0, 2.0, 0], P(1, 5, 2.0), P(6, 1, 2.0), P(0, 0, 1.0), P(5, 4, 0.5)], {(0, 0): 1.0, (5, 4): 0.5}))
    # a negative depth becomes 0: as the last write (1, 1), as the minimum of a group (2, 2), alone (3, 3)
    cases.append((NEG, [N(1, 1, 8.0), N(1, 1, 2.0), N(2, 2, 2.0), N(2, 2, 12.0), N(3, 3, 2.0), N(4, 1, 6.0)], {(4, 1): 2.0}))
    # x < 0 (it would land on (1, 1) with depth -2), NaN and inf points: dropped
    cases.append((EYE, [P(1, 1, -2.0), [nan, 1, 1, 0], [2.0, nan, 1, 0], [2.0, 2.0, nan, 0], [inf, 2.0, 1.0, 0], [2.0, 2.0, inf, 0],
                        P(4, 2, 2.0)], {(4, 2): 2.0}))
    # no point at all, between frames whose counts differ
    cases.append((EYE, np.zeros((0, 4)), {}))
    cases.append((EYE, [P(0, 1, 2.0)], {(0, 1): 2.0}))
    want = np.stack([expect(hits) for _, _, hits in cases])
    np.testing.assert_array_equal(VD.depth_maps([np.asarray(c, np.float32).reshape(-1, 4) for _, c, _ in cases], [m for m, _, _ in cases],
                                                h, w), want)
    got = run(ops, [c for _, c, _ in cases], [m for m, _, _ in cases])
    for b in range(len(cases)):
        np.testing.assert_array_equal(got[b], want[b], err_msg="case %d" % b)
    # a batch of three with 0 points in the middle
    three = run(ops, [cases[0][1], cases[-2][1], cases[6][1]], [EYE] * 3)
    np.testing.assert_array_equal(three, want[[0, -2, 6]])


def test_non_integer_bounds(ops):
    """The reference tests against img_width / ratio, a float: 4.5 keeps column 4, 4.0 drops it."""
    pts = [P(5, 4, 2.0), P(1, 3, 4.0)]
    np.testing.assert_array_equal(run(ops, [pts], [EYE], lims=(5.5, 4.5))[0], expect({(5, 4): 2.0, (1, 3): 4.0}))
    np.testing.assert_array_equal(run(ops, [pts], [EYE], lims=(5.0, 4.0))[0], expect({(1, 3): 4.0}))
    np.testing.assert_array_equal(VD.depth_map(np.array(pts, np.float32), EYE, h, w, 5.0, 4.0), expect({(1, 3): 4.0}))


def test_bad_arguments(ops):
    lib = _lib.load()
    assert lib.dn_velo_depth_workspace_bytes(1, 6, 1, 10) == 0 and lib.dn_velo_depth_workspace_bytes(1, 6, 5, 10) == 16 * 25 + 4 * 30
    with pytest.raises(_lib.DispnetHipError, match="bounds"):
        run(ops, [[P(1, 1, 2.0)]], [EYE], lims=(6.0, 5.5))
    with pytest.raises(_lib.DispnetHipError):
        run(ops, [[P(1, 1, 2.0)]], [EYE], shape=(6, 1), lims=(6.0, 1.0))
    t = torch.zeros(64, dtype=torch.float64, device=DEV)
    assert lib.dn_velo_depth(None, t.data_ptr(), 4, t.data_ptr(), 1, 6, 5, 6.0, 5.0, t.data_ptr(), 512, t.data_ptr(), None) == -1   # DN_ERR_BAD_ARG
    assert lib.dn_velo_depth(t.data_ptr(), t.data_ptr(), 1, t.data_ptr(), 1, 6, 5, 6.0, 5.0, t.data_ptr(), 8, t.data_ptr(), None) == -3  # workspace


@pytest.mark.parametrize("shape", [(375, 1242), (120, 400)])
def test_synthetic_scene_equals_kitti_gt_golden(ops, golden, shape):
    cloud, M = VD.kitti_gt_inputs(_golden_generator())
    want = VD.golden_map(golden("kitti_gt"), shape)
    got = run(ops, [cloud], [M], shape)
    print("%dx%d: %d pixels differ" % (shape[0], shape[1], int((got[0] != want).sum())))
    np.testing.assert_array_equal(got[0], want)
    again = run(ops, [cloud], [M], shape)
    assert got.tobytes() == again.tobytes()                             # two runs of the same call: identical bytes


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    base = tmp_path_factory.mktemp("kitti_raw_gpu")
    return {"root": T.write_tree(base / "raw"), "held": T.write_test_scenes(base / "test_scenes.txt"), "base": base}


@pytest.mark.parametrize("ratio", [1, 2])
def test_fabricated_clouds_batch_of_four(ops, tree, ratio):
    loader = KP.KittiRawLoader(tree["root"], img_height=16, img_width=48, get_depth=True, depth_size_ratio=ratio)
    shape, lims = loader.depth_shape()
    scenes = [s for drive in loader.scenes[:3:2] for s in loader.collect_scenes(drive)]       # two dates x two cameras
    assert len(scenes) == 4
    clouds = [KP.read_cloud(loader.velo_file(s, k)) for k, s in enumerate(scenes)]
    Ms = [loader.velo2im(s) for s in scenes]
    want = VD.depth_maps(clouds, Ms, shape[0], shape[1], *lims)
    assert (want > 0).sum() > 100 * 4 // ratio
    np.testing.assert_array_equal(run(ops, clouds, Ms, shape, lims), want)


def test_resize_u8_ragged_batch_equals_pil(ops):
    from PIL import Image
    frames = [T.frame("2011_09_26", "0801", "02", 1), T.frame("2011_09_26", "0801", "03", 2, 37, 121), T.frame("2011_09_28", "0801", "02", 3, 16, 48)]
    got = ops.resize(frames, (16, 48)).cpu().numpy()
    for b, f in enumerate(frames):
        want = np.asarray(Image.fromarray(f).resize((48, 16), Image.BILINEAR))
        bad = int((got[b] != want).sum())
        print("frame %d %s: %d bytes differ" % (b, f.shape[:2], bad))
        assert bad == 0
    np.testing.assert_array_equal(got[2], frames[2])
    both, _ = KP.device_batch(ops, frames, (16, 48))
    np.testing.assert_array_equal(both, got)
    # dn_imresize_u8 keeps its stretch
    u8, _ = ops.imresize(frames, (16, 48), want_u8=True)
    u8 = u8.cpu().numpy()
    for b, f in enumerate(frames):
        want = f if f.shape[:2] == (16, 48) else KE.imresize_bilinear(f.astype(np.float32), (16, 48))
        np.testing.assert_array_equal(u8[b], want)
    assert (u8[0] != got[0]).any()


def test_prepare_train_data_device_chain_equals_host_chain(tree):
    import prepare_train_data
    common = [tree["root"], "--height", "16", "--width", "48", "--with-depth", "--with-pose", "--test-scenes", tree["held"], "--readers", "2"]
    host, device = str(tree["base"] / "host"), str(tree["base"] / "device")
    prepare_train_data.main(common + ["--dump-root", host, "--host-chain"])
    p = subprocess.run([sys.executable, os.path.join(ROOT, "prepare_train_data.py")] + common + ["--dump-root", device, "--batch", "3"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    files = lambda root: sorted(os.path.relpath(os.path.join(d, n), root) for d, _, names in os.walk(root) for n in names)
    assert files(device) == files(host) and len(files(host)) == 2 + 4 * (2 + 2 * 3)
    for name in files(host):
        assert open(os.path.join(host, name), "rb").read() == open(os.path.join(device, name), "rb").read(), name
