"""monodepth2's colour jitter on the device, bit for bit everywhere: dn_colour_jitter_sums / _normalize_flip / _u8
against the host chain -- data.colour_jitter_u8 (Pillow itself; tests/test_colour_jitter_host.py holds it to the arithmetic of
tests/colour_jitter.py), then data.Transform.apply -- in all 24 orders, on degenerate frames, on every colour, on ragged sizes; the
identity for unjittered samples; two launches per batch; ShardLoader(color_aug=True) against the host chain replayed with the same draws,
with and without scale_crop; and train.py --color-aug, supervised on the tape and with monodepth2's objective on the plain frames."""
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

import colour_jitter as CJ  # noqa: E402
import scale_crop as SC  # noqa: E402
from supervised_dispnet_amd import _lib, data as D, shards as S  # noqa: E402
from tests.cases import make_scene_folders  # noqa: E402

DEV = torch.device("cuda:0")
CHUNKS = 64
MEAN, STD = D.normalization(imagenet=True)


@pytest.fixture(scope="module", autouse=True)
def _leave_the_stream_pool_where_it_was():
    """torch.cuda.Stream() hands out a pool of streams per device round-robin, and tests later in the suite depend on the slot their
    step's stream lands on (a GraphedStep / TapedStep on a weight-gradient side stream does not replay the eager
    step).  The loaders and tapes of this module draw some twenty streams; the tests behind it shall find the slot they would have found
    without it.  Before: one whole turn of the pool (ends one slot past where it began: the handles in order).  After: draw until the
    slot in front of the first one has been handed out, so that the next draw is again the first."""
    turn, seen = [], set()
    while True:
        h = torch.cuda.Stream(device=DEV).cuda_stream
        if h in seen:
            break
        turn.append(h)
        seen.add(h)
    assert h == turn[0] and 2 <= len(turn) <= 64, (len(turn), "the stream pool is not a round-robin turn")
    yield
    for _ in range(len(turn)):                               # the next draw is slot 1 if nothing was drawn; any slot otherwise
        if torch.cuda.Stream(device=DEV).cuda_stream == turn[-1]:
            break
    else:
        raise AssertionError("the stream pool did not come round to the slot this module started from")


def _table(params):
    tb = np.zeros((len(params), S.COLOUR_PARAMS), dtype=np.int32)
    for row, p in zip(tb, params):
        S.colour_params_row(p, row)
    return tb


def _device(u8, params, flips=None, plain=True, floats=True, bytes_=True):
    """u8 [N, B, H, W, 3], one set of parameters per sample -> (augmented fp32, plain fp32, jittered uint8) from the device, as tensors"""
    N, B, H, W, _ = u8.shape
    d_u8, d_cp = torch.from_numpy(u8).to(DEV), torch.from_numpy(_table(params)).to(DEV)
    d_fl = torch.from_numpy(np.asarray(flips, dtype=np.uint8)).to(DEV) if flips is not None else None
    sums = torch.empty((N * B, CHUNKS), dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    aug = pl = out8 = None
    _lib.call("dn_colour_jitter_sums", d_u8.data_ptr(), d_cp.data_ptr(), N, B, H, W, sums.data_ptr(), st)
    if floats:
        aug = torch.full((N, B, 3, H, W), float("nan"), dtype=torch.float32, device=DEV)
        pl = torch.full((N, B, 3, H, W), float("nan"), dtype=torch.float32, device=DEV) if plain else None
        _lib.call("dn_colour_jitter_normalize_flip", d_u8.data_ptr(), d_fl.data_ptr() if d_fl is not None else None, d_cp.data_ptr(),
                  sums.data_ptr(), N, B, H, W, (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD), aug.data_ptr(),
                  pl.data_ptr() if plain else None, st)
    if bytes_:
        out8 = torch.full((N, B, H, W, 3), 77, dtype=torch.uint8, device=DEV)
        _lib.call("dn_colour_jitter_u8", d_u8.data_ptr(), d_cp.data_ptr(), sums.data_ptr(), N, B, H, W, out8.data_ptr(), st)
    torch.cuda.synchronize()
    return aug, pl, out8


def _normalize_flip(u8, flips):
    """dn_u8_normalize_flip of every image row of u8 [N, B, H, W, 3]: what the loader computes without the jitter"""
    N, B, H, W, _ = u8.shape
    d_u8 = torch.from_numpy(u8).to(DEV)
    d_fl = torch.from_numpy(np.asarray(flips, dtype=np.uint8)).to(DEV)
    md, sd = torch.tensor(MEAN, device=DEV), torch.tensor(STD, device=DEV)
    out = torch.empty((N, B, 3, H, W), dtype=torch.float32, device=DEV)
    for n in range(N):
        _lib.call("dn_u8_normalize_flip", d_u8[n].data_ptr(), d_fl.data_ptr(), B, H, W, 3, md.data_ptr(), sd.data_ptr(), (C.c_float * 3)(*MEAN),
                  (C.c_float * 3)(*STD), out[n].data_ptr(), 3 * H * W, H * W, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


def _host(u8, params, flips):
    """the host chain: Pillow's jitter of every frame, then Transform.apply's flip and normalise -> (fp32 [N, B, 3, H, W], uint8 like u8)"""
    N, B, H, W, _ = u8.shape
    t = D.Transform(MEAN, STD, flip=True)
    want8 = np.empty_like(u8)
    want = torch.empty((N, B, 3, H, W), dtype=torch.float32)
    gt = np.zeros((H, W), dtype=np.float32)
    for b in range(B):
        for n in range(N):
            want8[n, b] = D.colour_jitter_u8(u8[n, b], params[b])
        tensors = t.apply([want8[n, b].astype(np.float32) for n in range(N)], gt, None, bool(flips[b]))[0]
        for n in range(N):
            want[n, b] = tensors[n]
    return want, want8


def _check(u8, params, flips):
    aug, plain, out8 = _device(u8, params, flips)
    want, want8 = _host(u8, params, flips)
    bad8 = np.argwhere((out8.cpu().numpy() != want8).any(axis=(2, 3, 4)))
    assert bad8.size == 0, "uint8: (image, sample) %r, parameters %r" % (bad8[:4].tolist(), [params[b] for _, b in bad8[:4]])
    bad = np.argwhere((aug.cpu().view(torch.int32) != want.view(torch.int32)).numpy().any(axis=(2, 3, 4)))
    assert bad.size == 0, "fp32: (image, sample) %r, parameters %r" % (bad[:4].tolist(), [params[b] for _, b in bad[:4]])
    assert torch.equal(plain.view(torch.int32), _normalize_flip(u8, flips).view(torch.int32))     # the plain output ALWAYS is the old kernel's


# ------------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("flip0", [0, 1])
@pytest.mark.parametrize("H,W", [(5, 7), (8, 16)], ids=["5x7", "8x16"])
def test_all_24_orders(H, W, flip0):
    """one sample per permutation, three images each; 3 W = 21 bytes per row takes the one-pixel path, 8 x 16 the four-pixel one"""
    u8 = CJ.random_frames((3, 24, H, W), 100 * H + W)
    flips = (np.arange(24) + flip0) % 2
    _check(u8, CJ.order_params(), flips)


@pytest.mark.parametrize("H,W", [(6, 10), (4, 8)], ids=["6x10", "4x8"])
def test_degenerate_frames(H, W):
    """black (max == 0: the grey branch, no division), white, a constant colour (its contrast mean is its own luma), a pure primary; the
    hue shifts 0, 1, 128 and 255, hue first and hue behind contrast"""
    frames = CJ.degenerate_frames(H, W)
    u8, params = [], []
    for f in frames:
        for shift in (0, 1, 128, 255):
            for order in ((3, 0, 1, 2), (1, 2, 3, 0)):
                u8.append(f)
                params.append((order, 1.1, 0.9, 1.15, shift))
    u8 = np.stack(u8)[None]
    _check(u8, params, np.zeros(len(params), dtype=np.uint8))


def test_every_colour_through_the_hue_round_trip():
    """1 x 2 x 4096 x 4096: every RGB triple, hue only (the three factors are exactly 1: those blends are the identity), shifts 0 and 231,
    against Pillow.  Shift 0 is no shortcut: the result differs from the input exactly where Pillow's round trip does."""
    from PIL import Image
    a = CJ.all_colours()
    shifts = (0, 231)
    params = [((3, 0, 1, 2), 1.0, 1.0, 1.0, s) for s in shifts]
    u8 = np.stack([a, a])[None]
    _, _, out8 = _device(u8, params, floats=False)
    got = out8.cpu().numpy()
    for b, s in enumerate(shifts):
        h, sat, v = Image.fromarray(a).convert("HSV").split()
        nh = ((np.asarray(h, dtype=np.int32) + s) % 256).astype(np.uint8)
        want = np.asarray(Image.merge("HSV", (Image.fromarray(nh), sat, v)).convert("RGB"))
        assert np.array_equal(got[0, b], want), "shift %d: %d bytes differ" % (s, int((got[0, b] != want).sum()))
        if s == 0:
            assert (want != a).any() and np.array_equal(got[0, b] != a, want != a)


@pytest.mark.parametrize("N,B,H,W", [(2, 3, 23, 37), (1, 1, 40, 136), (1, 2, 128, 416)], ids=["3x23x37", "1x40x136", "2x128x416"])
def test_ragged_and_training_sizes(N, B, H, W):
    u8 = CJ.random_frames((N, B, H, W), H + W)
    params = CJ.order_params(H)[5:5 + B]
    if B > 1:
        params[1] = None                                 # an unjittered sample between jittered ones
    _check(u8, params, np.arange(B) % 2)


@pytest.mark.parametrize("H,W", [(5, 7), (8, 16)], ids=["5x7", "8x16"])
def test_unjittered_samples_are_the_old_kernel(H, W):
    u8 = CJ.random_frames((2, 4, H, W), 3)
    flips = np.array([0, 1, 1, 0], dtype=np.uint8)
    aug, plain, out8 = _device(u8, [None] * 4, flips)
    want = _normalize_flip(u8, flips)
    assert torch.equal(aug.view(torch.int32), want.view(torch.int32)) and torch.equal(plain.view(torch.int32), want.view(torch.int32))
    assert np.array_equal(out8.cpu().numpy(), u8)
    aug2, none, _ = _device(u8, [None] * 4, flips, plain=False, bytes_=False)         # without the plain output
    assert none is None and torch.equal(aug2.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("B", [2, 24])
def test_two_launches_per_batch(B):
    """counted by the library's launch tape, recorded only (as tests/test_gpu_mono2.py counts a step's launches)"""
    lib = _lib.load()
    u8 = CJ.random_frames((3, B, 8, 16), B)
    params = (CJ.order_params() * 2)[:B]
    _device(u8, params, np.zeros(B, dtype=np.uint8), bytes_=False)
    tape = lib.dn_tape_begin()
    assert tape, _lib.last_error()
    try:
        _device(u8, params, np.zeros(B, dtype=np.uint8), bytes_=False)
        assert lib.dn_tape_end(tape) == 0
        assert lib.dn_tape_launches(tape) == 2
    finally:
        lib.dn_tape_free(tape)


# ------------------------------------------------------------------------------------------------------------------ loader
def _shards(tmp_path, h=16, w=32):
    root = make_scene_folders(tmp_path / "kitti", frames=6, h=h, w=w)
    S.write_shards(str(root), str(tmp_path / "sh"), train=True, sequence_length=3)
    return root, S.ShardSet(str(tmp_path / "sh"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("scale_crop", [False, True], ids=["flip", "flip+scale_crop"])
def test_shard_loader_equals_the_host_chain(tmp_path, scale_crop):
    """One pass of 5-tuples (two full batches and the ragged tail) against the host chain replayed with the same draws: the jitter
    (Pillow), then Transform.apply with the flip [and the crop]; ._dn_plain against the same chain without the jitter."""
    _, st = _shards(tmp_path)
    H, W = st.H, st.W
    mean, std = D.normalization()
    kw = dict(batch_size=5, device=DEV, mean=mean, std=std, flip=True, shuffle=False, with_refs=True, drop_last=False, scale_crop=scale_crop)
    loader = S.ShardLoader(st, flip_rng=random.Random(11), aug_rng=np.random.RandomState(5), color_aug=True, keep_plain=True,
                           colour_rng=np.random.RandomState(7), **kw)
    base = S.ShardLoader(st, flip_rng=random.Random(11), aug_rng=np.random.RandomState(5), **kw)
    host = D.Transform(mean, std, flip=True, scale_crop=scale_crop)
    fdraws, adraws, cdraws = random.Random(11), np.random.RandomState(5), np.random.RandomState(7)
    seen = jittered = 0
    for (img, refs, k, kinv, gt), (bimg, brefs, bk, bkinv, bgt) in zip(loader, base):
        # flips, crops, intrinsics and ground truth are the unjittered loader's; so are the plain frames
        assert torch.equal(k, bk) and torch.equal(kinv, bkinv) and torch.equal(gt, bgt)
        assert torch.equal(img._dn_plain, bimg) and all(torch.equal(r._dn_plain, br) for r, br in zip(refs, brefs))
        assert not hasattr(bimg, "_dn_plain")
        for j in range(img.shape[0]):
            tgt, ref_idx, scene = st.samples[seen]
            flip = fdraws.random() < 0.5
            crop = SC.draws(adraws, H, W) if scale_crop else None
            params = D.draw_colour_jitter(cdraws)
            jittered += params is not None
            frames = [np.asarray(st.frames[i]) for i in [tgt] + ref_idx]
            imgs, wgt, kk = host.apply([D.colour_jitter_u8(f, params).astype(np.float32) for f in frames], np.asarray(st.depth[tgt]),
                                       st.intrinsics[scene].copy(), flip, crop)
            assert torch.equal(img[j].cpu(), imgs[0]) and torch.equal(gt[j].cpu(), wgt), (seen, flip, crop, params)
            for r in range(len(ref_idx)):
                assert torch.equal(refs[r][j].cpu(), imgs[1 + r]), (seen, r, flip, crop, params)
            assert np.array_equal(_bits(k[j].cpu().numpy()), _bits(kk))
            seen += 1
    assert seen == len(st) == 12 and 0 < jittered < 12


@pytest.mark.parametrize("scale_crop", [False, True], ids=["flip", "flip+scale_crop"])
def test_the_jitter_draws_are_a_stream_of_their_own(tmp_path, scale_crop):
    """Same --seed with and without the jitter: the same flips and crops (ground truth, intrinsics, plain frames); set_epoch moves the
    jitter draws; color_aug=False stages no table and consumes no draw."""
    _, st = _shards(tmp_path)

    def first(epoch, **kw):
        ld = S.ShardLoader(st, 6, DEV, shuffle=True, seed=4, with_refs=True, scale_crop=scale_crop, **kw)
        ld.set_epoch(epoch)
        return next(iter(ld)), ld

    (a, _), (b, _), (c, _) = first(1, color_aug=True, keep_plain=True), first(1), first(2, color_aug=True)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    assert torch.equal(a[0]._dn_plain, b[0]) and all(torch.equal(x._dn_plain, y) for x, y in zip(a[1], b[1]))
    assert not torch.equal(a[0], b[0])                                          # some sample of the six was jittered
    (a2, _) = first(1, color_aug=True, keep_plain=True)
    assert torch.equal(a[0], a2[0]) and not hasattr(c[0], "_dn_plain")
    rng = np.random.RandomState(9)
    state = rng.get_state()[1].copy()
    d, ld = first(1, color_aug=False, keep_plain=True, colour_rng=rng)
    assert torch.equal(d[0], b[0]) and not hasattr(d[0], "_dn_plain") and "cp" not in ld._ring[0]
    assert np.array_equal(rng.get_state()[1], state)


# ------------------------------------------------------------------------------------------------------------------ train.py
def _log_rows(out):
    runs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs]
    full = [r for r in runs if r.endswith("progress_log_full.csv")][0]
    rows = [l.split("\t") for l in open(full).read().strip().splitlines()]
    return [[float(v) for v in r] for r in rows[1:]]


def test_train_cli_color_aug_supervised_on_the_tape(tmp_path, capsys):
    import train
    root, _ = _shards(tmp_path, h=64, w=96)
    out = tmp_path / "run"
    train.main([str(root), "--shards", str(tmp_path / "sh"), "--color-aug", "--epochs", "1", "--epoch-size", "2", "-b", "4", "--save-root", str(out),
                "--print-freq", "100", "--network", "disp_vgg_BN", "--loss", "L1", "--with-gt"])
    text = capsys.readouterr().out
    assert "--tape:" in text and "bit for bit" in text and "eager launches (" not in text, text[-600:]
    vals = np.array(_log_rows(out))
    assert vals.shape[0] == 2 and np.isfinite(vals).all() and (vals[:, 0] > 0).all()


def test_train_cli_color_aug_monodepth2_loss_reads_the_plain_frames(tmp_path):
    """two iterations of --unsupervised --monodepth2 --min-reprojection --color-aug from shards; the first step's loss is monodepth2_loss on
    the PLAIN frames with both networks fed the jittered ones -- the same launches on the same inputs, so the same fp32 value -- and not
    the value with the jittered frames in the loss"""
    import train
    import supervised_dispnet_amd.loss_functions as LF
    import supervised_dispnet_amd.models as models
    import supervised_dispnet_amd.networks as networks
    import supervised_dispnet_amd.utils as U
    root, _ = _shards(tmp_path, h=64, w=96)
    wdir = tmp_path / "mono2_weights"
    wdir.mkdir()
    torch.manual_seed(5)
    enc = networks.ResnetEncoder(18, False)
    torch.save(enc.state_dict(), str(wdir / "encoder.pth"))
    torch.save(networks.DepthDecoder(enc.num_ch_enc).state_dict(), str(wdir / "depth.pth"))
    torch.save(networks.PoseCNN(num_input_frames=2).state_dict(), str(wdir / "pose.pth"))
    out = tmp_path / "run"
    argv = [str(root), "--shards", str(tmp_path / "sh"), "--color-aug", "--unsupervised", "--monodepth2", "--min-reprojection", "--network",
            "disp_res_18", "--pretrained-disp", str(wdir), "--pretrained-exppose", str(wdir / "pose.pth"), "-b", "4", "--epochs", "1",
            "--epoch-size", "2", "-s", "1e-3", "--with-gt", "--seed", "3", "--save-root", str(out), "--print-freq", "100"]
    train.main(argv)
    rows = _log_rows(out)
    assert len(rows) == 2 and np.isfinite(np.array(rows)).all()
    # the first step again, from the same weights and the same loader
    args = train.build_parser().parse_args(argv)
    disp_net = train.create_disp_net(args, models, networks, DEV, U).train()
    pose = networks.PoseCNN(num_input_frames=2).to(DEV)
    pose.load_state_dict(torch.load(str(wdir / "pose.pth"), map_location=DEV))
    pose.train()
    mean, std = D.normalization(args.imagenet_normalization, args.monodepth2)
    loader = S.ShardLoader(str(tmp_path / "sh"), 4, DEV, mean=mean, std=std, flip=True, shuffle=True, seed=args.seed, with_refs=True,
                           color_aug=True, keep_plain=True)
    loader.set_epoch(0)
    tgt, refs, K, Kinv, _gt = train._to_device_batch(next(iter(loader)), DEV, True, True)
    ptgt, prefs = train.plain_frames(tgt, refs)
    assert ptgt is not tgt and not torch.equal(ptgt, tgt)                       # this seed jitters two of the first four samples
    plain = float(train.min_reprojection_objective(args, LF, disp_net, pose, ptgt, prefs, K, Kinv, net_tgt=tgt, net_refs=refs).item())
    jit = float(train.min_reprojection_objective(args, LF, disp_net, pose, tgt, refs, K, Kinv).item())
    print("first step: logged %.9g, plain frames in the loss %.9g, jittered frames in the loss %.9g" % (rows[0][0], plain, jit))
    assert rows[0][0] == plain
    assert rows[0][0] != jit
