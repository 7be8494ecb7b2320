"""Pose evaluation on the GPU (eval_pose.py, supervised_dispnet_amd/pose_eval.py, csrc/dn_poseeval.hip): the snippet
gather bit for bit against numpy fp32, the two metric kernels against the longdouble restatement and against numpy fp64 within the DERIVED
bounds of tests/pose_eval_audit.py, the batched forward of the three pose networks against one snippet at a time, and eval_pose.py end to
end as the device chain and as --host-chain on both dataset layouts.  pytest -m gpu.

Gather shapes: one pixel; a plane of 6 (no vector group); 35 pixels (not a multiple of 4: the short last group); 65 snippets of 24 pixels
(vector path, more than one block); the evaluation's own 128 x 416.  The ring holds K + 1 frames, so every table wraps.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import pose_eval_audit as A  # noqa: E402
import pose_eval_tree as T  # noqa: E402
import eval_pose  # noqa: E402
import supervised_dispnet_amd.models as models  # noqa: E402
import supervised_dispnet_amd.networks as networks  # noqa: E402
from supervised_dispnet_amd import _lib, pose_eval as PE  # noqa: E402

DEV = torch.device("cuda:0")
BAD_ARG = -1
SENTINEL = -777.0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f3(v):
    return (C.c_float * 3)(*v)


def pose_close(got, want, what):
    """the tolerance tests/test_gpu_pose_net.py holds pose outputs to"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, tol = float(np.abs(got - want).max()), 1e-3 * float(np.abs(want).max()) + 1e-7
    print("%s: max|got - want| %.3e, tolerance %.3e (max|want| %.3e)" % (what, err, tol, float(np.abs(want).max())))
    assert float(np.abs(want).max()) > 0 and err <= tol, what


# ------------------------------------------------------------------------------------------------------------------ gather
GATHER_SHAPES = ((1, 2, 1, 1), (2, 3, 2, 3), (3, 5, 5, 7), (65, 5, 4, 6), (2, 2, 128, 416))


def _gather_inputs(N, K, H, W):
    rng = np.random.RandomState(1000 * N + 100 * K + H + W)
    R = K + 1
    ring = rng.randint(0, 256, (R, H, W, 3)).astype(np.uint8)
    ring.reshape(-1)[:2] = (0, 255)
    idx = (np.arange(N)[:, None] + rng.permutation(K)[None, :]).astype(np.int32)     # overlapping snippets, as consecutive targets are
    idx[N // 2] = idx[N // 2, 0]                                                       # one frame repeated through a whole snippet
    idx[-1, -1] = 7 * R + 2                                                            # far past the ring
    return ring, idx, R


def _gather_want(ring, idx, R, mean, std):
    N, K = idx.shape
    x = ring[idx % R].astype(np.float32)                                               # [N, K, H, W, 3]
    x = ((x / np.float32(255)) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    return np.ascontiguousarray(np.transpose(x, (0, 1, 4, 2, 3))).reshape(N, 3 * K, ring.shape[1], ring.shape[2])


@pytest.mark.parametrize("protocol", PE.PROTOCOLS)
@pytest.mark.parametrize("N,K,H,W", GATHER_SHAPES)
def test_snippet_gather_is_bit_exact(N, K, H, W, protocol):
    ring, idx, R = _gather_inputs(N, K, H, W)
    mean, std = PE.normalization(protocol)
    want = _gather_want(ring, idx, R, mean, std)
    d_ring, d_idx = torch.from_numpy(ring).to(DEV), torch.from_numpy(idx).to(DEV)
    buf = torch.full((want.size + 1,), SENTINEL, dtype=torch.float32, device=DEV)
    for shift in (0, 1):                                   # an aligned destination, and one a float off (pixel by pixel at any size)
        buf.fill_(SENTINEL)
        dst = buf[shift:shift + want.size]
        _lib.call("dn_snippet_gather", d_ring.data_ptr(), R, d_idx.data_ptr(), N, K, H, W, _f3(mean), _f3(std), dst.data_ptr(), _stream())
        got = dst.cpu().numpy().reshape(want.shape)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (shift, float(np.abs(got - want).max()))
        assert float(buf[want.size if shift == 0 else 0]) == SENTINEL


def test_snippet_gather_wraps_negative_indices():
    ring, idx, R = _gather_inputs(2, 3, 2, 3)
    idx[0, 0] = -1
    mean, std = PE.normalization("sfmlearner")
    d_ring, d_idx = torch.from_numpy(ring).to(DEV), torch.from_numpy(idx).to(DEV)
    dst = torch.empty((2, 9, 2, 3), dtype=torch.float32, device=DEV)
    _lib.call("dn_snippet_gather", d_ring.data_ptr(), R, d_idx.data_ptr(), 2, 3, 2, 3, _f3(mean), _f3(std), dst.data_ptr(), _stream())
    assert np.array_equal(dst.cpu().numpy(), _gather_want(ring, idx, R, mean, std))          # numpy's % wraps the same way


def test_bad_arguments_are_refused_without_a_launch():
    lib = _lib.load()
    ring = torch.zeros((3, 2, 3, 3), dtype=torch.uint8, device=DEV)
    idx = torch.zeros((2, 2), dtype=torch.int32, device=DEV)
    dst = torch.full((2, 6, 2, 3), SENTINEL, dtype=torch.float32, device=DEV)
    m, s = _f3([0.5] * 3), _f3([0.5] * 3)
    good = [ring.data_ptr(), 3, idx.data_ptr(), 2, 2, 2, 3, m, s, dst.data_ptr(), _stream()]
    for pos, bad in ((0, None), (2, None), (9, None), (7, None), (8, None), (1, 0), (3, 0), (4, 0), (5, 0), (6, -1)):
        args = list(good)
        args[pos] = bad
        assert lib.dn_snippet_gather(*args) == BAD_ARG, pos
        assert "dn_snippet_gather" in _lib.last_error()
    pose = torch.zeros((2, 2, 6), dtype=torch.float32, device=DEV)
    gt = torch.zeros((2, 3, 3, 4), dtype=torch.float64, device=DEV)
    out = torch.full((2, 2), SENTINEL, dtype=torch.float64, device=DEV)
    good = [pose.data_ptr(), 0, gt.data_ptr(), 2, 3, out.data_ptr(), _stream()]
    for pos, bad in ((0, None), (2, None), (5, None), (1, 2), (1, -1), (3, 0), (4, 1), (4, 34)):
        args = list(good)
        args[pos] = bad
        assert lib.dn_pose_eval_sfm(*args) == BAD_ARG, pos
        assert "dn_pose_eval_sfm" in _lib.last_error()
    Q = torch.zeros((2, 4, 4), dtype=torch.float64, device=DEV)
    out1 = torch.full((2,), SENTINEL, dtype=torch.float64, device=DEV)
    good = [pose.data_ptr(), Q.data_ptr(), 2, 5, out1.data_ptr(), _stream()]
    for pos, bad in ((0, None), (1, None), (4, None), (2, 0), (3, 1), (3, 65)):
        args = list(good)
        args[pos] = bad
        assert lib.dn_pose_eval_mono2(*args) == BAD_ARG, pos
        assert "dn_pose_eval_mono2" in _lib.last_error()
    torch.cuda.synchronize()
    assert float(dst.min()) == SENTINEL == float(dst.max()) and float(out.max()) == SENTINEL == float(out1.max())


# ------------------------------------------------------------------------------------------------------------------ metric kernels
def _device_sfm(pose, gt, mode):
    N, L = gt.shape[:2]
    d_pose, d_gt = torch.from_numpy(np.ascontiguousarray(pose)).to(DEV), torch.from_numpy(np.ascontiguousarray(gt)).to(DEV)
    outs = []
    for _ in range(2):
        out = torch.full((N, 2), SENTINEL, dtype=torch.float64, device=DEV)
        _lib.call("dn_pose_eval_sfm", d_pose.data_ptr(), PE.ROTATION_MODES[mode], d_gt.data_ptr(), N, L, out.data_ptr(), _stream())
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.int64), outs[1].view(np.int64)), "two runs differ"
    return outs[0]


def _device_mono2(pose, Q, track=PE.TRACK_LENGTH):
    P = len(Q)
    d_pose, d_Q = torch.from_numpy(np.ascontiguousarray(pose)).to(DEV), torch.from_numpy(np.ascontiguousarray(Q)).to(DEV)
    outs = []
    for _ in range(2):
        out = torch.full((P,), SENTINEL, dtype=torch.float64, device=DEV)
        _lib.call("dn_pose_eval_mono2", d_pose.data_ptr(), d_Q.data_ptr(), P, track, out.data_ptr(), _stream())
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.int64), outs[1].view(np.int64)), "two runs differ"
    return outs[0]


@pytest.mark.parametrize("kind", A.SFM_KINDS)
def test_pose_eval_sfm_is_inside_the_bound(kind):
    for (N, L) in A.SFM_SIZES:
        pose, gt, mode = A.sfm_case(kind, N, L)
        ref, bnd = A.sfm_reference(kind, N, L)
        host = PE.sfm_metric(pose, gt, mode)
        got = _device_sfm(pose, gt, mode)
        shares = [A.share(got[:, c], ref[:, c], bnd[:, c]) for c in (0, 1)] + [A.share(got[:, c], host[:, c], bnd[:, c]) for c in (0, 1)]
        print("sfm %-18s N=%3d L=%d %-5s  share of the bound against longdouble: ATE %.4f RE %.4f;  against numpy fp64: ATE %.4f RE %.4f" % (
            (kind, N, L, mode) + tuple(shares)))
        assert max(shares) <= 1.0
        assert np.array_equal(got[:, 1] == 0, host[:, 1] == 0)
        if kind == "identity_rot":
            assert np.all(got[:, 1] == 0)                  # exactly
        if kind == "zeros":
            assert np.isnan(got[::2, 0]).all() and not np.isnan(got[1::2, 0]).any() and not np.isnan(got[:, 1]).any()


@pytest.mark.parametrize("kind", A.MONO2_KINDS)
def test_pose_eval_mono2_is_inside_the_bound(kind):
    for P in A.MONO2_SIZES:
        pose, Q = A.mono2_case(kind, P)
        ref, bnd = A.mono2_reference(kind, P)
        host = PE.mono2_metric(pose, Q)
        got = _device_mono2(pose, Q)
        s_ref, s_host = A.share(got, ref, bnd), A.share(got, host, bnd)
        print("mono2 %-10s P=%2d  share of the bound against longdouble %.4f, against numpy fp64 %.4f;  NaN windows %d" % (
            kind, P, s_ref, s_host, int(np.isnan(got).sum())))
        assert max(s_ref, s_host) <= 1.0
        if kind == "zeros":
            assert np.isnan(got[P // 2:]).all() and not np.isnan(got[:P // 2]).any()


def test_pose_eval_mono2_other_track_lengths():
    pose, Q = A.mono2_case("well", 5)
    for track in (2, 3, 9):
        ref, bnd = A.mono2(pose, Q, track)
        assert A.share(_device_mono2(pose, Q, track), ref, bnd) <= 1.0


# ------------------------------------------------------------------------------------------------------------------ batched forward
@pytest.fixture(scope="module")
def sequence():
    """9 frames of 64 x 96 resident on the device as the ring of a 9-frame batch, and the same frames normalised on the host."""
    frames = np.stack([T.frame("fw", k, 64, 96) for k in range(9)])
    return frames, torch.from_numpy(frames).to(DEV)


def _dense(sequence, table, protocol):
    frames, ring = sequence
    table = np.asarray(table, dtype=np.int32)
    N, K = table.shape
    mean, std = PE.normalization(protocol)
    dense = torch.empty((N, 3 * K, 64, 96), dtype=torch.float32, device=DEV)
    _lib.call("dn_snippet_gather", ring.data_ptr(), 9, torch.from_numpy(table).to(DEV).data_ptr(), N, K, 64, 96, _f3(mean), _f3(std),
              dense.data_ptr(), _stream())
    host = np.stack([np.concatenate([PE.host_frame(frames[i], None, mean, std) for i in row]) for row in table])
    assert np.array_equal(dense.cpu().numpy(), host)       # the operand of the device chain is the host chain's, bit for bit
    return dense


def _seeded(make):
    torch.manual_seed(20240521)
    net = make()
    if hasattr(net, "init_weights"):
        net.init_weights()
    return net.to(DEV).eval()


def test_poseexpnet_takes_five_frame_snippets_as_one_operand(sequence):
    net = _seeded(lambda: models.PoseExpNet(nb_ref_imgs=4, output_exp=False))
    table = [PE.sfm_operand_order(row) for row in PE.snippet_indices(9, 5)]
    assert len(table) == 5
    dense = _dense(sequence, table, "sfmlearner")
    assert dense.shape == (5, 15, 64, 96)
    got = PE.forward_poses(net, dense)
    assert got.shape == (5, 4, 6)
    want = torch.cat([PE.forward_poses(net, dense[i:i + 1].contiguous()) for i in range(5)])
    pose_close(got.cpu().numpy(), want.cpu().numpy(), "PoseExpNet(4), batch 5 against one snippet at a time")
    with pytest.raises(NotImplementedError):               # the limit of forward(target, refs) stays where it is
        net(dense[:, :3].contiguous(), [dense[:, 3 * k:3 * k + 3].contiguous() for k in range(1, 5)])


def test_poseexpnet_dense_operand_equals_forward(sequence):
    net = _seeded(lambda: models.PoseExpNet(nb_ref_imgs=2, output_exp=False))
    table = [PE.sfm_operand_order(row) for row in PE.snippet_indices(9, 3)]
    dense = _dense(sequence, table, "sfmlearner")
    got = PE.forward_poses(net, dense)
    with torch.no_grad():
        _, want = net(dense[:, :3].contiguous(), [dense[:, 3:6].contiguous(), dense[:, 6:9].contiguous()])
    pose_close(got.cpu().numpy(), want.cpu().numpy(), "PoseExpNet(2), dense operand against forward(target, refs)")
    single = torch.cat([PE.forward_poses(net, dense[i:i + 1].contiguous()) for i in range(len(table))])
    pose_close(got.cpu().numpy(), single.cpu().numpy(), "PoseExpNet(2), batch 7 against one snippet at a time")


@pytest.mark.parametrize("name", ("posecnn", "resnet18"))
def test_pair_networks_batched_against_single(sequence, name):
    net = _seeded((lambda: networks.PoseCNN(2)) if name == "posecnn" else (lambda: networks.PoseResnet(18)))
    dense = _dense(sequence, [(i, i + 1) for i in range(8)], "monodepth2")
    got = PE.forward_poses(net, dense)
    assert got.shape == (8, 1, 6)
    want = torch.cat([PE.forward_poses(net, dense[i:i + 1].contiguous()) for i in range(8)])
    pose_close(got.cpu().numpy(), want.cpu().numpy(), "%s, batch 8 against one pair at a time" % name)


# ------------------------------------------------------------------------------------------------------------------ end to end
E2E_SEQUENCES = (("09", 12), ("10", 7))
E2E_SIZE, NET_SIZE = (20, 60), (16, 48)


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    root = tmp_path_factory.mktemp("eval_pose")
    trees = {"odometry": T.write_odometry(str(root / "odometry"), E2E_SEQUENCES, E2E_SIZE),
             "folders": T.write_folders(str(root / "folders"), E2E_SEQUENCES, E2E_SIZE, "jpg")}
    torch.manual_seed(7)
    exp = models.PoseExpNet(nb_ref_imgs=2, output_exp=False)
    exp.init_weights()
    torch.save({"state_dict": exp.state_dict()}, str(root / "exp_pose.pth.tar"))
    torch.save(networks.PoseCNN(2).state_dict(), str(root / "pose.pth"))
    return root, trees


def _run(capsys, argv):
    capsys.readouterr()
    results = eval_pose.main(argv)
    return results, capsys.readouterr().out


@pytest.mark.parametrize("fmt", ("odometry", "folders"))
@pytest.mark.parametrize("protocol", PE.PROTOCOLS)
def test_eval_pose_end_to_end(e2e, capsys, protocol, fmt):
    root, trees = e2e
    sfm = protocol == "sfmlearner"
    weights = ["--pretrained-posenet", str(root / "exp_pose.pth.tar")] if sfm else ["--pretrained-posenet", str(root / "pose.pth"), "--pose-model", "posecnn"]
    common = weights + ["--dataset-dir", trees[fmt], "--dataset-format", fmt, "--sequences", "09", "10", "--img-height", str(NET_SIZE[0]),
                        "--img-width", str(NET_SIZE[1])]
    tag = "%s_%s" % (protocol, fmt)
    dev_dump, host_dump, out_dir = str(root / (tag + "_dev.npy")), str(root / (tag + "_host.npy")), str(root / (tag + "_out"))
    dev_res, dev_out = _run(capsys, common + ["--batch", "4", "--readers", "2", "--dump-poses", dev_dump, "--output-dir", out_dir])
    host_res, host_out = _run(capsys, common + ["--host-chain", "--dump-poses", host_dump])
    dev_raw, host_raw = np.load(dev_dump), np.load(host_dump)
    assert dev_raw.dtype == np.float32 and dev_raw.shape == ((10 + 5, 2, 6) if sfm else (11 + 6, 6))
    # 1. the two chains hand the network the same frames: their raw outputs agree as a batched forward agrees with a single one
    pose_close(dev_raw, host_raw, "%s: dumped poses, device chain against --host-chain" % tag)
    # 2. the device chain's metrics are the host metric of ITS OWN dumped poses, within the audit bounds
    pos = 0
    for name, n in E2E_SEQUENCES:
        files, poses = PE.read_sequence(trees[fmt], name, fmt)
        if sfm:
            idx = PE.snippet_indices(n, 3)
            gt = np.stack([PE.compensated_poses(poses, row) for row in idx])
            raw = dev_raw[pos:pos + len(idx)]
            ref, bnd = A.sfm(raw, gt, "euler")
            host = PE.sfm_metric(raw, gt, "euler")
            shares = [A.share(dev_res[name][:, c], host[:, c], bnd[:, c]) for c in (0, 1)] + [A.share(dev_res[name][:, c], ref[:, c], bnd[:, c]) for c in (0, 1)]
            lines = PE.format_sfm(dev_res[name])
        else:
            Q = PE.gt_local_transforms(poses)
            raw = dev_raw[pos:pos + n - 1]
            ref, bnd = A.mono2(raw, Q)
            host = PE.mono2_metric(raw, Q)
            shares = [A.share(dev_res[name], host, bnd), A.share(dev_res[name], ref, bnd)]
            lines = PE.format_mono2(dev_res[name])
        pos += len(raw)
        print("%s sequence %s: shares of the bound %s" % (tag, name, ["%.4f" % s for s in shares]))
        assert max(shares) <= 1.0
        assert dev_res[name].shape == host_res[name].shape and np.isfinite(dev_res[name]).all()
        for line in lines:
            assert line in dev_out.splitlines(), (line, dev_out)
        assert "sequence %s: %d frames" % (name, n) in dev_out and "sequence %s: %d frames" % (name, n) in host_out
    assert pos == len(dev_raw)
    saved = np.load(os.path.join(out_dir, "predictions.npy"))
    assert saved.shape == ((15, 3, 3, 4) if sfm else (17, 4, 4)) and np.array_equal(saved, PE.predictions(protocol, dev_raw))
    assert ("Trajectory error" in dev_out) != sfm and ("mean \t" in dev_out) == sfm
