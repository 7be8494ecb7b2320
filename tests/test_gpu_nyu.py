"""NYU Depth v2 on the MI355X: the HIP chain (csrc/dn_nyu.hip) against the reference's goldens and against scipy directly, the
loader against the per-sample CPU chain, and train.py --dataset nyu end to end on a fabricated tree."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import nyu_chain as NC  # noqa: E402
DEV = torch.device("cuda:0")
STD = np.asarray(NC.NYUD_STD, dtype=np.float64)


@pytest.fixture(scope="module")
def nyu():
    import __graft_entry__
    __graft_entry__.build(only_library=True)
    from supervised_dispnet_amd import nyu as N
    return N


def _check(img, depth, want_img, want_depth, min_equal=0.99):
    """>= 99 % of the elements bit-identical; every element within 4 ulp at the scale of the value before normalisation."""
    img, depth = np.asarray(img), np.asarray(depth)
    assert img.shape == want_img.shape and depth.shape == want_depth.shape
    assert np.isfinite(img).all() and np.isfinite(depth).all()
    eq = (np.sum(img == want_img) + np.sum(depth == want_depth)) / float(img.size + depth.size)
    assert eq >= min_equal, "only %.4f of the elements bit-identical" % eq
    tol_rgb = 4 * 2.0 ** -23 * 255.0 / STD
    err_rgb = np.abs(img.astype(np.float64) - want_img).reshape(img.shape[0], 3, -1).max(axis=(0, 2))
    assert (err_rgb <= tol_rgb).all(), (err_rgb, tol_rgb)
    tol_d = 4 * 2.0 ** -23 * max(1.0, float(np.abs(want_depth).max()))
    assert np.abs(depth.astype(np.float64) - want_depth).max() <= tol_d


def _augment(nyu, raws, draws, size):
    raw = torch.from_numpy(np.ascontiguousarray(np.stack(raws))).to(DEV)
    par = torch.from_numpy(nyu.params_array(draws)).to(DEV)
    img, depth = nyu.augment_batch(raw, par, size=size)
    torch.cuda.synchronize()
    return img.cpu().numpy(), depth.cpu().numpy()


@pytest.mark.parametrize("name", ["small", "exact", "full"])
def test_train_kernels_match_reference_goldens(nyu, golden, name):
    g = golden("nyu_transform")
    H0, W0, th, tw = (int(v) for v in g[name + "_shape"])
    raws = [NC.raw_sample(H0, W0, "nyu:%s:%d" % (name, k)) for k in g[name + "_seeds"]]
    draws = [(bool(d[0]), d[1], int(d[2]), int(d[3]), d[4], d[5]) for d in g[name + "_draws"]]
    img, depth = _augment(nyu, raws, draws, (th, tw))
    assert img.shape == (len(raws), 3, th, tw) and np.isfinite(img).all() and np.isfinite(depth).all()
    rows = g[name + "_rows"]
    _check(img[:, :, rows], depth[:, rows], g[name + "_img"], g[name + "_depth"])


def test_val_kernel_matches_reference_goldens(nyu, golden):
    g = golden("nyu_transform")
    H, W = (int(v) for v in g["val_shape"])
    ims = torch.from_numpy(NC.raw_test_images(2, "nyu:val", H, W)).to(DEV)
    out = nyu.resize_batch(ims, size=g["val_img"].shape[2:]).cpu().numpy()
    _check(out, np.zeros((1, 1)), g["val_img"], np.zeros((1, 1)))


@pytest.mark.parametrize("flip", [0, 1])
def test_prefilter_matches_scipy_spline_filter(nyu, flip):
    from supervised_dispnet_amd import _lib
    raws = np.stack([NC.raw_sample(44, 60, "pf:%d" % k) for k in range(2)])
    raw = torch.from_numpy(raws).to(DEV)
    par = torch.from_numpy(nyu.params_array([(flip, 0.0, 0, 0, 1.0, 1.0)] * 2)).to(DEV)
    coef, mm = nyu.new_workspace(2, 44, 60, DEV)
    _lib.call("dn_nyu_prefilter", raw.data_ptr(), par.data_ptr(), 2, 44, 60, coef.data_ptr(), mm.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    coef, mm = coef.cpu().numpy(), mm.cpu().numpy()
    for b in range(2):
        assert mm[b, :, 0].min() == raws[b].min() and mm[b, :, 1].max() == raws[b].max()
        for ch in range(4):
            plane = raws[b, ch][:, ::-1] if flip else raws[b, ch]
            ref = ndi.spline_filter(plane.astype(np.float64), 3, mode="mirror")
            assert np.abs(coef[b, ch] - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("angle", [5.0, -5.0, 45.0, -45.0])
def test_rotation_matches_scipy_rotate(nyu, angle):
    """s = 1, gain 1 and a raw of exactly 256x352: the chain reduces to the clipped rotation + Normalize; +-45 degrees exercise the
    zero corners."""
    raws = [NC.raw_sample(256, 352, "rot:%d" % k) for k in range(2)]
    img, depth = _augment(nyu, raws, [(k == 1, angle, 0, 0, 1.0, 1.0) for k in range(2)], (256, 352))
    want_img, want_depth = [], []
    for k, raw in enumerate(raws):
        hwc = raw.transpose(1, 2, 0)
        if k == 1:
            hwc = hwc[:, ::-1, :]
        r = np.clip(ndi.rotate(hwc, angle, reshape=False, axes=(0, 1), mode="constant"), hwc.min(), hwc.max())
        want_img.append(NC.normalize(np.clip(r[:, :, :3].astype(np.float64), 0, 255).astype(np.float32).transpose(2, 0, 1)))
        want_depth.append(r[:, :, 3])
    _check(img, depth, np.stack(want_img), np.stack(want_depth))
    if abs(angle) == 45.0:                  # at least two corners fall outside the rotated source: value 0 before normalisation
        zero = np.float32((0 - np.float32(0.485)) / np.float32(0.229))
        assert ((img[:, 0, [0, 0, -1, -1], [0, -1, 0, -1]] == zero).sum(axis=1) >= 2).all()


def test_val_resize_matches_scipy_zoom(nyu):
    ims = NC.raw_test_images(2, "zoom")
    out = nyu.resize_batch(torch.from_numpy(ims).to(DEV)).cpu().numpy()
    want = np.stack([NC.normalize(np.ascontiguousarray(ndi.zoom(im.transpose(1, 2, 0), (320 / 480, 448 / 640, 1), order=1)
                                                      .transpose(2, 0, 1))) for im in ims])
    _check(out, np.zeros((1, 1)), want, np.zeros((1, 1)))


def _tree(root, n_train, H0, W0, n_test, H=480, W=640):
    from test_nyu_host import make_tree
    return make_tree(root, n_train=n_train, H0=H0, W0=W0, n_test=n_test, H=H, W=W, tag="e2e")


def test_loader_matches_the_per_sample_chain_and_splits_over_ranks(nyu, tmp_path):
    root = _tree(str(tmp_path), 8, 300, 400, 3, 96, 128)
    one = nyu.NyuLoader(root, 4, DEV, train=True, seed=5)
    one.set_epoch(1)
    order = list(one.sampler)
    batches = [(i.cpu().numpy(), d.cpu().numpy()) for i, d in one]
    assert len(batches) == 2 and batches[0][0].shape == (4, 3, 256, 352) and batches[0][1].shape == (4, 256, 352)
    ts = nyu.NyuTrainSet(root)
    for (img, depth), idxs in zip(batches, order):
        for j, i in enumerate(idxs):
            p = nyu.draw_params(np.random.RandomState(nyu.sample_seed(5, 1, i)), 300, 400)
            wi, wd = NC.train_chain(ts[i], p)
            _check(img[j:j + 1], depth[j:j + 1], wi[None], wd[None])
    halves = []
    for rank in range(2):
        ld = nyu.NyuLoader(root, 2, DEV, train=True, seed=5, rank=rank, world=2)
        ld.set_epoch(1)
        halves.append([(i.cpu().numpy(), d.cpu().numpy()) for i, d in ld])
    for b, (img, depth) in enumerate(batches):
        np.testing.assert_array_equal(np.concatenate([halves[0][b][0], halves[1][b][0]]), img)
        np.testing.assert_array_equal(np.concatenate([halves[0][b][1], halves[1][b][1]]), depth)
    val = nyu.NyuLoader(root, 2, DEV, train=False)
    got = [(i.cpu().numpy(), d.cpu().numpy()) for i, d in val]
    assert [g[0].shape[0] for g in got] == [2, 1]
    vs = nyu.NyuTestSet(root)
    for k in range(3):
        img, depth = got[k // 2][0][k % 2], got[k // 2][1][k % 2]
        assert img.shape == (3, 320, 448) and depth.shape == (96, 128)
        np.testing.assert_array_equal(depth, vs[k][1])
        want = NC.normalize(np.stack([NC.zoom_restated(vs[k][0][c], 320, 448) for c in range(3)]))
        _check(img[None], np.zeros((1, 1)), want[None], np.zeros((1, 1)))


@pytest.mark.parametrize("tape", [True, False])
def test_train_py_nyu_end_to_end(tmp_path, tape):
    root = _tree(str(tmp_path / "data"), 8, 320, 448, 4)
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), root, "--dataset", "nyu", "--with-gt", "-b4", "--epochs", "1", "--epoch-size", "2",
           "--network", "disp_vgg_BN", "--loss", "L1", "--save-root", str(tmp_path / "ck"), "--print-freq", "1"]
    if not tape:
        cmd.append("--no-tape")
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "training crop 256x352" in out and "8 samples found" in out and "4 samples found" in out
    if tape:
        assert "replay == eager step" in out, out[-4000:]
    m = re.findall(r"\* Avg abs_diff : (\S+), abs_rel : (\S+), sq_rel : (\S+), rmse : (\S+)", out)
    assert m and all(np.isfinite(float(v.rstrip(","))) for v in m[-1]), out[-4000:]
    ck = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path / "ck") for f in fs if f == "dispnet_checkpoint.pth.tar"]
    assert len(ck) == 1
