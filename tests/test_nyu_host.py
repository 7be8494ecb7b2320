"""NYU Depth v2 on the host (no GPU): the CPU restatement of the reference's transform chain against the goldens the reference itself
produced (tests/golden/make_nyu_goldens.py), the draw order, the scipy facts the HIP kernels rely on, the on-disk dataset classes and
train.py's refusals."""
import os
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import nyu_chain as NC  # noqa: E402
from supervised_dispnet_amd import nyu  # noqa: E402

CASES = ("small", "exact", "full")


def _case(g, name):
    H0, W0, th, tw = (int(v) for v in g[name + "_shape"])
    raws = [NC.raw_sample(H0, W0, "nyu:%s:%d" % (name, k)) for k in g[name + "_seeds"]]
    return raws, (th, tw)


@pytest.mark.parametrize("name", CASES)
def test_chain_restatement_matches_reference_goldens(golden, name):
    g = golden("nyu_transform")
    raws, size = _case(g, name)
    for j, raw in enumerate(raws):
        d = g[name + "_draws"][j]
        img, depth = NC.train_chain(raw, (bool(d[0]), d[1], int(d[2]), int(d[3]), d[4], d[5]), size)
        rows = g[name + "_rows"]
        np.testing.assert_array_equal(img[:, rows], g[name + "_img"][j])
        np.testing.assert_array_equal(depth[rows], g[name + "_depth"][j])


def test_val_restatement_matches_reference_goldens(golden):
    g = golden("nyu_transform")
    H, W = (int(v) for v in g["val_shape"])
    ims = NC.raw_test_images(2, "nyu:val", H, W)
    for j in range(2):
        np.testing.assert_array_equal(NC.val_chain(ims[j], size=g["val_img"].shape[2:]), g["val_img"][j])


@pytest.mark.parametrize("name", CASES)
def test_draw_params_reproduce_the_reference_draws(golden, name):
    g = golden("nyu_transform")
    H0, W0, th, tw = (int(v) for v in g[name + "_shape"])
    for j, k in enumerate(g[name + "_seeds"]):
        rs = np.random.RandomState(int(k))
        p = nyu.draw_params(rs, H0, W0, (th, tw))
        np.testing.assert_array_equal(np.asarray(p, dtype=np.float64), g[name + "_draws"][j])
        assert rs.uniform() == g[name + "_next"][j]        # same draw count: both leave the stream at the same place
    assert set(g[name + "_ndraws"]) == ({4} if name == "exact" else {6})
    assert g[name + "_rows"][-1] == th - 1 and (name == "full" or len(g[name + "_rows"]) == th)


@pytest.mark.parametrize("shape", [(256, 400), (300, 352), (255, 400), (300, 351), (200, 200)])
def test_mixed_and_small_sizes_are_refused(shape):
    with pytest.raises(ValueError, match="cannot be cropped"):
        nyu.draw_params(np.random.RandomState(0), shape[0], shape[1])


def test_draws_stay_in_the_reference_ranges():
    for k in range(200):
        flip, angle, r0, c0, s, mult = nyu.draw_params(np.random.RandomState(k), 320, 448)
        assert -5 <= angle < 5 and 0 <= r0 < 320 - 256 and 0 <= c0 < 448 - 352 and 1 <= s < 1.5 and 0.8 <= mult < 1.2
    assert nyu.sample_seed(1, 2, 3) == ((1 * 1000003 + 2) * 1000003 + 3) % (1 << 32)
    assert len({nyu.sample_seed(0, e, i) for e in range(3) for i in range(100)}) == 300


# ----------------------------------------------------------------------------- scipy facts the kernels implement
def test_prefilter_is_scipy_spline_filter_with_mirror_boundaries():
    raw = NC.raw_sample(44, 60, "facts")
    for ch in range(5):
        plane = raw[ch].astype(np.float64)
        ref = ndi.spline_filter(plane, 3, mode="mirror")
        np.testing.assert_array_equal(ndi.spline_filter(plane, 3, mode="constant"), ref)
        got = NC.spline_prefilter(raw[ch])
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("angle", [3.3, -4.9, 45.0, -45.0, 17.0])
def test_rotate_restatement_matches_scipy(angle):
    raw = NC.raw_sample(44, 60, "facts")
    for ch in range(5):
        ref64 = ndi.rotate(raw[ch].astype(np.float64), angle, reshape=False, mode="constant")
        got = NC.rotate_restated(raw[ch], angle)
        assert np.abs(got - ref64).max() <= 1e-13 * max(1.0, np.abs(raw[ch]).max())
        # float32 input: scipy returns exactly float32(fp64 result)
        np.testing.assert_array_equal(ndi.rotate(raw[ch], angle, reshape=False, mode="constant"), ref64.astype(np.float32))


def test_rotate_of_hwc_is_per_plane():
    im = NC.raw_sample(44, 60, "facts").transpose(1, 2, 0)
    r = ndi.rotate(im, 4.0, reshape=False, axes=(0, 1), mode="constant")
    for ch in range(5):
        np.testing.assert_array_equal(r[:, :, ch], ndi.rotate(np.ascontiguousarray(im[:, :, ch]), 4.0, reshape=False, mode="constant"))


def test_zoom_restatement_matches_scipy():
    img = NC.raw_test_images(1, "facts")[0]
    for ch in range(3):
        np.testing.assert_array_equal(NC.zoom_restated(img[ch], 320, 448), ndi.zoom(img[ch], (320 / 480, 448 / 640), order=1))
    hwc = img.transpose(1, 2, 0)
    z = ndi.zoom(hwc, (320 / 480, 448 / 640, 1), order=1)
    assert z.shape == (320, 448, 3) and z.dtype == np.float32
    for ch in range(3):
        np.testing.assert_array_equal(z[:, :, ch], NC.zoom_restated(img[ch], 320, 448))


def test_warp_zoom_reads_toward_the_top_left_corner():
    a = np.arange(4 * 6 * 2, dtype=np.float64).reshape(4, 6, 2)
    w = NC.warp_zoom(a, 1.0)
    np.testing.assert_array_equal(w, a)
    w = NC.warp_zoom(a, 2.0)
    np.testing.assert_array_equal(w[0, 0], a[0, 0])
    np.testing.assert_allclose(w[1, 1], (a[0, 0] + a[0, 1] + a[1, 0] + a[1, 1]) / 4)
    np.testing.assert_array_equal(w[2, 2], a[1, 1])


# ----------------------------------------------------------------------------- on-disk layout
def make_tree(root, n_train=3, H0=44, W0=60, n_test=2, H=48, W=64, tag="tree"):
    """A fabricated DATA tree in the reference's layout (names deliberately not created in sorted order)."""
    tdir = nyu.train_dir(root)
    os.makedirs(tdir, exist_ok=True)
    for i in reversed(range(n_train)):
        np.save(os.path.join(tdir, "%05d.npy" % i), NC.raw_sample(H0, W0, "%s:%d" % (tag, i)))
    vdir = nyu.test_dir(root)
    os.makedirs(vdir, exist_ok=True)
    np.save(os.path.join(vdir, "images.npy"), NC.raw_test_images(n_test, tag, H, W))
    np.save(os.path.join(vdir, "depths.npy"), NC.raw_test_depths(n_test, tag, H, W))
    return root


def test_dataset_classes_on_a_fabricated_tree(tmp_path):
    root = make_tree(str(tmp_path), H0=300, W0=400)
    ts = nyu.NyuTrainSet(root)
    assert len(ts) == 3 and (ts.H0, ts.W0) == (300, 400)
    assert [os.path.basename(p) for p in ts.file_paths] == ["00000.npy", "00001.npy", "00002.npy"]
    np.testing.assert_array_equal(ts[1], NC.raw_sample(300, 400, "tree:1"))
    vs = nyu.NyuTestSet(root)
    assert len(vs) == 2 and (vs.H, vs.W) == (48, 64) and isinstance(vs.images, np.memmap)
    img, depth = vs[1]
    np.testing.assert_array_equal(img, NC.raw_test_images(2, "tree", 48, 64)[1])
    np.testing.assert_array_equal(depth, NC.raw_test_depths(2, "tree", 48, 64)[1, 0])


def test_dataset_refuses_bad_samples(tmp_path):
    root = make_tree(str(tmp_path / "a"), H0=256, W0=400)
    with pytest.raises(ValueError, match="cannot be cropped"):
        nyu.NyuTrainSet(root)
    root = make_tree(str(tmp_path / "b"), H0=300, W0=400)
    np.save(os.path.join(nyu.train_dir(root), "00009.npy"), NC.raw_sample(310, 400, "odd"))
    ts = nyu.NyuTrainSet(root)
    with pytest.raises(ValueError, match="differs from the first sample"):
        ts[3]
    with pytest.raises(FileNotFoundError):
        nyu.NyuTrainSet(str(tmp_path / "missing"))


def test_params_array_layout():
    p = nyu.params_array([(True, -2.5, 3, 7, 1.25, 0.9), (False, 4.0, 0, 0, 1.0, 1.1)])
    assert p.dtype == np.float64 and p.shape == (2, 8)
    np.testing.assert_array_equal(p[0], [1, -2.5, 3, 7, 1.25, 0.9, 0, 0])
    with pytest.raises(ValueError):
        nyu.params_array([(False, 0.0, 0, 0, 0.5, 1.0)])


# ----------------------------------------------------------------------------- train.py
@pytest.mark.parametrize("extra,msg", [(["--with-gt", "--shards", "S"], "--shards"), (["--with-gt", "--unsupervised"], "--unsupervised"),
                                       ([], "--with-gt")])
def test_train_refuses_what_the_nyu_loader_cannot_serve(extra, msg):
    import train
    with pytest.raises(SystemExit) as e:
        train.main(["DATA", "--dataset", "nyu"] + extra)
    text = str(e.value.code)
    assert msg in text and "\n" not in text


def test_train_nyu_checks_leave_synthetic_and_kitti_alone():
    import train
    p = train.build_parser()
    for argv in (["D", "--dataset", "nyu", "--synthetic", "8"], ["D", "--dataset", "nyu", "--synthetic", "8", "--unsupervised"],
                 ["D", "--shards", "S"], ["D", "--dataset", "nyu", "--with-gt"]):
        train.check_dataset_args(p.parse_args(argv))
