"""Random scale-and-crop on the device: dn_scale_crop_minmax / dn_scale_crop_u8 / dn_scale_crop_depth are BIT-EXACT
against the numpy restatement of tests/scale_crop.py (which tests/test_scale_crop_host.py holds to Pillow), ShardLoader(scale_crop=True)
batches equal the host chain data.Transform(scale_crop=True) fed the same draws, scale_crop=False changes nothing, a scaled size below
the crop is refused on the host, and train.py --scale-crop runs."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import scale_crop as SC  # noqa: E402
from supervised_dispnet_amd import _lib, data as D, inference as I, shards as S  # noqa: E402
from tests.cases import make_scene_folders  # noqa: E402

DEV = torch.device("cuda:0")
CHUNKS = 64


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _run_kernels(u8, gt, flips, crops, mean, std):
    """u8 [N, B, H, W, 3], gt [B, H, W], flips [B], crops [(sh, sw, oy, ox)] -> (fp32 [N, B, 3, H, W], fp32 [B, H, W]) from the device."""
    N, B, H, W, _ = u8.shape
    table, taps = I.scale_crop_table(H, W, crops)
    hw = np.ascontiguousarray([c[:2] for c in crops], dtype=np.int32)
    d_u8, d_gt, d_fl = torch.from_numpy(u8).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(flips).to(DEV)
    d_tb = torch.from_numpy(table).to(DEV)
    mm_u8 = torch.empty((N * B, CHUNKS, 2), dtype=torch.int32, device=DEV)
    mm_gt = torch.empty((B, CHUNKS, 2), dtype=torch.float32, device=DEV)
    out = torch.full((N, B, 3, H, W), float("nan"), dtype=torch.float32, device=DEV)
    ogt = torch.full((B, H, W), float("nan"), dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    hwp = hw.ctypes.data_as(C.c_void_p)
    _lib.call("dn_scale_crop_minmax", d_u8.data_ptr(), d_gt.data_ptr(), N, B, H, W, mm_u8.data_ptr(), mm_gt.data_ptr(), st)
    _lib.call("dn_scale_crop_u8", d_u8.data_ptr(), d_fl.data_ptr(), N, B, H, W, mm_u8.data_ptr(), d_tb.data_ptr(), hwp, taps,
              (C.c_float * 3)(*mean), (C.c_float * 3)(*std), out.data_ptr(), st)
    _lib.call("dn_scale_crop_depth", d_gt.data_ptr(), d_fl.data_ptr(), B, H, W, mm_gt.data_ptr(), d_tb.data_ptr(), hwp, taps, ogt.data_ptr(), st)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ogt.cpu().numpy()


def _check(u8, gt, flips, crops, mean, std):
    out, ogt = _run_kernels(u8, gt, flips, crops, mean, std)
    N, B = u8.shape[:2]
    for b in range(B):
        sh, sw, oy, ox = crops[b]
        for n in range(N):
            _, want = SC.image(u8[n, b], bool(flips[b]), sh, sw, oy, ox, mean, std)
            assert np.array_equal(_bits(out[n, b]), _bits(want)), "image %d of sample %d: %r, flip %d" % (n, b, crops[b], flips[b])
        want = SC.depth(gt[b], bool(flips[b]), sh, sw, oy, ox)
        assert np.array_equal(_bits(ogt[b]), _bits(want)), "depth of sample %d: %r, flip %d" % (b, crops[b], flips[b])


@pytest.mark.parametrize("H,W", [(20, 70), (24, 37)])
def test_kernels_equal_the_restatement(H, W):
    """B = 6 samples of 3 images; the sizes cross a tile edge (16 x 64) in both axes and are multiples of neither 4 nor the tile."""
    r = np.random.RandomState(H * 100 + W)
    N, B = 3, 6
    mh, mw = int(1.15 * H), int(1.15 * W)
    crops = [(H, W, 0, 0),                       # scale exactly 1 on both axes: byte-scale only
             (H, mw, 0, (mw - W) // 2),          # x only
             (mh, W, mh - H, 0),                 # y only
             (mh, mw, 0, 0),                     # both at the largest scale, offset 0
             (mh, mw, mh - H, mw - W),           # ... and the largest offset
             (H + 1, W + 2, 1, 1)]
    flips = np.array([0, 1, 0, 1, 0, 1], dtype=np.uint8)
    u8 = r.randint(20, 240, (N, B, H, W, 3)).astype(np.uint8)
    u8[1, 2] = 93                                # one constant frame
    u8[0, 3, 0, 0], u8[0, 3, -1, -1] = 0, 255    # one frame that spans the whole range already
    gt = (r.rand(B, H, W) * 80 + 1).astype(np.float32)
    gt[0] = 0                                    # one all-zero map
    gt[1] *= r.rand(H, W) < 0.05                 # one with 5 % non-zero pixels
    gt[4] *= r.rand(H, W) < 0.3
    mean, std = D.normalization(imagenet=True)
    _check(u8, gt, flips, crops, mean, std)


def test_kernels_equal_the_restatement_at_the_training_size():
    r = np.random.RandomState(3)
    N, B, H, W = 3, 4, 128, 416
    dr = np.random.RandomState(8)
    crops = [SC.draws(dr, H, W)[2:] for _ in range(B - 1)] + [(int(1.15 * H), int(1.15 * W), int(1.15 * H) - H, int(1.15 * W) - W)]
    flips = np.array([1, 0, 0, 1], dtype=np.uint8)
    u8 = r.randint(5, 250, (N, B, H, W, 3)).astype(np.uint8)
    gt = ((r.rand(B, H, W) * 79 + 1) * (r.rand(B, H, W) < 0.05)).astype(np.float32)
    _check(u8, gt, flips, crops, *D.normalization())


def _shards(tmp_path, h=16, w=32):
    root = make_scene_folders(tmp_path / "kitti", frames=6, h=h, w=w)
    S.write_shards(str(root), str(tmp_path / "sh"), train=True, sequence_length=3)
    return root, S.ShardSet(str(tmp_path / "sh"))


def test_shard_loader_equals_the_host_chain(tmp_path):
    """One pass of 5-tuples (two full batches and the ragged tail) against data.Transform(scale_crop=True).apply with the same draws."""
    _, st = _shards(tmp_path)
    H, W = st.H, st.W
    mean, std = D.normalization()
    loader = S.ShardLoader(st, batch_size=5, device=DEV, mean=mean, std=std, flip=True, shuffle=False, with_refs=True, drop_last=False,
                           flip_rng=random.Random(11), scale_crop=True, aug_rng=np.random.RandomState(5))
    host = D.Transform(mean, std, flip=True, scale_crop=True)
    fdraws, adraws = random.Random(11), np.random.RandomState(5)
    seen, moved = 0, 0
    for img, refs, k, kinv, gt in loader:
        want_k = []
        for j in range(img.shape[0]):
            tgt, ref_idx, scene = st.samples[seen]
            flip = fdraws.random() < 0.5
            crop = SC.draws(adraws, H, W)
            moved += crop[2:4] != (H, W)
            frames = [np.asarray(st.frames[i]).astype(np.float32) for i in [tgt] + ref_idx]
            imgs, wgt, kk = host.apply(frames, np.asarray(st.depth[tgt]), st.intrinsics[scene].copy(), flip, crop)
            assert torch.equal(img[j].cpu(), imgs[0]) and torch.equal(gt[j].cpu(), wgt), (seen, flip, crop)
            for r in range(len(ref_idx)):
                assert torch.equal(refs[r][j].cpu(), imgs[1 + r]), (seen, r, flip, crop)
            assert np.array_equal(_bits(k[j].cpu().numpy()), _bits(kk)), (seen, flip, crop)
            want_k.append(kk)
            seen += 1
        assert np.array_equal(_bits(kinv.cpu().numpy()), _bits(np.linalg.inv(np.stack(want_k))))
    assert seen == len(st) == 12 and len(loader) == 3 and moved > 0
    # the private generators: reproducible from (seed, rank, epoch), moved by set_epoch
    def first(epoch, seed=4):
        ld = S.ShardLoader(st, 4, DEV, shuffle=False, seed=seed, with_refs=True, scale_crop=True)
        ld.set_epoch(epoch)
        return next(iter(ld))
    a, b, c = first(1), first(1), first(2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[4], b[4])
    assert not torch.equal(a[2], c[2])


def test_shard_loader_without_the_flag_is_unchanged(tmp_path):
    _, st = _shards(tmp_path)
    a = next(iter(S.ShardLoader(st, 5, DEV, flip=True, shuffle=False, with_refs=True, flip_rng=random.Random(2))))
    rng = np.random.RandomState(9)
    state = rng.get_state()[1].copy()
    ld = S.ShardLoader(st, 5, DEV, flip=True, shuffle=False, with_refs=True, flip_rng=random.Random(2), scale_crop=False, aug_rng=rng)
    b = next(iter(ld))
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    assert np.array_equal(rng.get_state()[1], state)             # no draw consumed
    assert "tb" not in ld._ring[0]                               # no table staged


def test_bad_arguments_are_refused_on_the_host():
    """A scaled size below the crop, or more taps than a table row holds: DN_ERR_BAD_ARG from the argument check, nothing launched."""
    lib = _lib.load()
    N, B, H, W = 1, 2, 20, 70
    table, taps = I.scale_crop_table(H, W, [(H, W, 0, 0)] * B)
    d_u8 = torch.zeros((N, B, H, W, 3), dtype=torch.uint8, device=DEV)
    d_gt = torch.zeros((B, H, W), dtype=torch.float32, device=DEV)
    d_tb = torch.from_numpy(table).to(DEV)
    mm_u8 = torch.zeros((N * B, CHUNKS, 2), dtype=torch.int32, device=DEV)
    mm_gt = torch.zeros((B, CHUNKS, 2), dtype=torch.float32, device=DEV)
    out = torch.full((N, B, 3, H, W), 7.0, device=DEV)
    ogt = torch.full((B, H, W), 7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    one = (C.c_float * 3)(1, 1, 1)
    for hw, t in (([[H, W], [H, W - 1]], taps), ([[H - 1, W], [H, W]], taps), ([[H, W], [H, W]], 4), ([[H, W], [H, W]], 0)):
        hw = np.ascontiguousarray(hw, dtype=np.int32)
        hwp = hw.ctypes.data_as(C.c_void_p)
        rc = lib.dn_scale_crop_u8(d_u8.data_ptr(), None, N, B, H, W, mm_u8.data_ptr(), d_tb.data_ptr(), hwp, t, one, one, out.data_ptr(), st)
        assert rc == -1 and b"dn_scale_crop_u8" in lib.dn_last_error()
        rc = lib.dn_scale_crop_depth(d_gt.data_ptr(), None, B, H, W, mm_gt.data_ptr(), d_tb.data_ptr(), hwp, t, ogt.data_ptr(), st)
        assert rc == -1 and b"dn_scale_crop_depth" in lib.dn_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ogt == 7.0).all())
    with pytest.raises(_lib.DispnetHipError):
        _lib.call("dn_scale_crop_u8", d_u8.data_ptr(), None, N, B, H, W, mm_u8.data_ptr(), d_tb.data_ptr(), hwp, 4, one, one, out.data_ptr(), st)


@pytest.mark.parametrize("extra", [["--network", "disp_vgg_BN", "--loss", "L1", "--with-gt"],
                                   ["--network", "disp_vgg_BN", "--unsupervised", "-s", "0.1"]], ids=["supervised", "unsupervised"])
def test_train_cli_scale_crop_from_shards(tmp_path, extra):
    """train.py DATA --shards S --scale-crop --epochs 1 --epoch-size 2 -b 4 on a tiny shard set, in process as tests/test_gpu_cli.py runs
    its command lines: two finite steps (supervised: through the launch tape; unsupervised: the 5-tuple with the adjusted intrinsics)."""
    import train
    root, _ = _shards(tmp_path, h=64, w=96)
    out = tmp_path / "run"
    train.main([str(root), "--shards", str(tmp_path / "sh"), "--scale-crop", "--epochs", "1", "--epoch-size", "2", "-b", "4",
                "--save-root", str(out), "--print-freq", "100"] + extra)
    runs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs]
    full = [r for r in runs if r.endswith("progress_log_full.csv")][0]
    rows = [l.split("\t") for l in open(full).read().strip().splitlines()]
    assert len(rows) == 1 + 2
    vals = np.array([[float(v) for v in r] for r in rows[1:]])
    assert np.isfinite(vals).all() and (vals[:, 0] > 0).all()
