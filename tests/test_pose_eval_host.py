"""Host side of the pose evaluation (supervised_dispnet_amd/pose_eval.py, eval_pose.py), no GPU: snippets and
compensated ground truth against the reference's own reader (tests/golden/pose_eval.npz, bit for bit), the numpy fp64 metrics against the
longdouble restatement within the derived bounds of tests/pose_eval_audit.py -- the check that the yardstick of the GPU tests is itself
inside the bound --, NaN propagation, the two dataset layouts, the command line's refusals and the printed formats."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import pose_eval_audit as A  # noqa: E402
import pose_eval_tree as T  # noqa: E402
import eval_pose  # noqa: E402
from supervised_dispnet_amd import pose_eval as PE  # noqa: E402


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    root = tmp_path_factory.mktemp("pose_eval")
    return T.write_odometry(str(root / "odometry")), T.write_folders(str(root / "folders"))


@pytest.mark.parametrize("L", T.GOLDEN_LENGTHS)
@pytest.mark.parametrize("name,n", T.GOLDEN_SEQUENCES)
def test_snippets_and_ground_truth_match_the_reference(golden, trees, name, n, L):
    g = golden("pose_eval")
    key = "%s:L%d" % (name, L)
    files, poses = PE.read_sequence(trees[0], name, "odometry")
    assert [os.path.relpath(f, trees[0]) for f in files] == list(g[key + ":files"]) and len(files) == n
    idx = PE.snippet_indices(n, L)
    assert idx.shape == g[key + ":indices"].shape and np.array_equal(idx, g[key + ":indices"])
    gt = np.array([PE.compensated_poses(poses, row) for row in idx]).reshape(-1, L, 3, 4)
    assert gt.dtype == np.float64 and np.array_equal(gt, g[key + ":poses"])        # bit for bit
    if len(idx):
        assert np.array_equal(gt[:, 0, :, 3], np.zeros((len(idx), 3)))


def test_golden_covers_both_lengths_and_an_empty_sequence(golden):
    g = golden("pose_eval")
    assert g["09:L3:indices"].shape == (5, 3) and g["09:L5:indices"].shape == (3, 5)
    assert g["10:L3:indices"].shape == (2, 3) and g["10:L5:indices"].shape == (0, 5)        # 4 frames hold no 5-frame snippet


def test_both_layouts_give_the_same_snippets(trees):
    for name, n in T.GOLDEN_SEQUENCES:
        fo, po = PE.read_sequence(trees[0], name, "odometry")
        ff, pf = PE.read_sequence(trees[1], name, "folders", ["png"])
        assert [os.path.basename(f) for f in fo] == [os.path.basename(f) for f in ff]
        assert np.array_equal(po, pf)
        for a, b in zip(fo, ff):
            assert np.array_equal(PE.read_frame(a), PE.read_frame(b))
        for L in T.GOLDEN_LENGTHS:
            for row in PE.snippet_indices(n, L):
                assert np.array_equal(PE.compensated_poses(po, row), PE.compensated_poses(pf, row))
    with pytest.raises(ValueError):
        PE.read_sequence(trees[0], "09", "video")


def test_operand_order_and_frame_arithmetic():
    assert PE.sfm_operand_order([4, 5, 6, 7, 8]) == [6, 4, 5, 7, 8] and PE.sfm_operand_order([0, 1, 2]) == [1, 0, 2]
    f = T.frame("09", 3, 8, 12)
    for protocol in PE.PROTOCOLS:
        mean, std = PE.normalization(protocol)
        x = PE.host_frame(f, (8, 12), mean, std)                     # already at the size: not resized
        assert x.dtype == np.float32 and x.shape == (3, 8, 12)
        want = (np.transpose(f, (2, 0, 1)).astype(np.float32) / np.float32(255) - np.float32(mean[0])) / np.float32(std[0])
        assert np.array_equal(x, want)
        assert np.array_equal(PE.host_frame(f, None, mean, std), x)
    assert PE.host_frame(f, (4, 6), *PE.normalization("sfmlearner")).shape == (3, 4, 6)
    assert float(np.abs(PE.host_frame(f, (8, 12), *PE.normalization("monodepth2"))).max()) <= 1.0


def test_library_function_errors_are_inside_the_table():
    got = A.measure_ulps(200000)
    print("ulp errors of numpy's fp64 functions against longdouble:", got)
    for name, v in got.items():
        assert v <= A.ULP[name], (name, v)


@pytest.mark.parametrize("kind", A.SFM_KINDS)
def test_numpy_sfm_metric_is_inside_the_bound(kind):
    for (N, L) in A.SFM_SIZES:
        pose, gt, mode = A.sfm_case(kind, N, L)
        ref, bnd = A.sfm_reference(kind, N, L)
        got = PE.sfm_metric(pose, gt, mode)
        assert got.shape == (N, 2) and got.dtype == np.float64
        s_ate, s_re = A.share(got[:, 0], ref[:, 0], bnd[:, 0]), A.share(got[:, 1], ref[:, 1], bnd[:, 1])
        print("sfm %-18s N=%3d L=%d %-5s  share of the bound: ATE %.4f  RE %.4f  (largest bound %.2e / %.2e)" % (
            kind, N, L, mode, s_ate, s_re, float(np.max(np.nan_to_num(bnd[:, 0]))), float(bnd[:, 1].max())))
        assert s_ate <= 1.0 and s_re <= 1.0
        assert np.array_equal(got[:, 1] == 0, np.asarray(ref[:, 1] == 0))
        if kind == "identity_rot":
            assert np.all(got[:, 1] == 0)
        if kind == "zeros":
            assert np.isnan(got[::2, 0]).all() and not np.isnan(got[1::2, 0]).any() and not np.isnan(got[:, 1]).any()
        if kind == "pi":
            assert float(ref[:, 1].max()) > 3.0 / L


@pytest.mark.parametrize("kind", A.MONO2_KINDS)
def test_numpy_mono2_metric_is_inside_the_bound(kind):
    for P in A.MONO2_SIZES:
        pose, Q = A.mono2_case(kind, P)
        ref, bnd = A.mono2_reference(kind, P)
        got = PE.mono2_metric(pose, Q)
        assert got.shape == (P,) and got.dtype == np.float64
        s = A.share(got, ref, bnd)
        print("mono2 %-10s P=%2d  share of the bound %.4f  NaN windows %d" % (kind, P, s, int(np.isnan(got).sum())))
        assert s <= 1.0
        if kind == "zeros":
            assert np.isnan(got[P // 2:]).all() and not np.isnan(got[:P // 2]).any()


def test_nan_is_propagated_into_the_mean():
    pose, gt, mode = A.sfm_case("zeros", 2, 5)
    errors = PE.sfm_metric(pose, gt, mode)
    assert np.isnan(errors[0, 0]) and not np.isnan(errors[1, 0])
    lines = PE.format_sfm(errors)
    assert "nan" in lines[2] and "nan" in lines[3]
    ates = PE.mono2_metric(*A.mono2_case("zeros", 1))
    assert np.isnan(ates).all() and "nan" in PE.format_mono2(ates)[0]


def test_windows_are_shorter_at_the_end():
    pose, Q = A.mono2_case("well", 5)
    ates = PE.mono2_metric(pose, Q)
    T4 = PE.transformation64(pose)
    for i, n in ((0, 4), (1, 4), (2, 3), (3, 2), (4, 1)):
        g, p = PE.dump_xyz(Q[i:i + n]), PE.dump_xyz(T4[i:i + n])
        assert g.shape == (n + 1, 3) and ates[i] == PE.compute_ate(g, p)
    assert np.allclose(PE.gt_local_transforms(A.trajectory(np.random.RandomState(1), 4))[:, 3], [0, 0, 0, 1])


def test_printed_formats():
    errors = np.array([[0.0123456, 0.002], [0.02, 0.004]])
    assert PE.format_sfm(errors) == ["Results", "\t {:>10}, {:>10}".format("ATE", "RE"),
                                     "mean \t {:10.4f}, {:10.4f}".format(0.0161728, 0.003), "std \t {:10.4f}, {:10.4f}".format(*errors.std(0))]
    assert PE.format_sfm(errors)[2] == "mean \t     0.0162,     0.0030"
    assert PE.format_mono2(np.array([0.01, 0.03])) == ["   Trajectory error: 0.020, std: 0.010"]


def test_command_line_refusals(tmp_path):
    ckpt = tmp_path / "pose.pth"
    ckpt.write_bytes(b"")
    folder = tmp_path / "mono"
    folder.mkdir()
    for argv, word in (
            (["--pretrained-posenet", str(ckpt), "--protocol", "monodepth2"], "sfmlearner"),
            (["--pretrained-posenet", str(ckpt), "--pose-model", "posecnn", "--protocol", "sfmlearner"], "monodepth2"),
            (["--pretrained-posenet", str(folder), "--pose-model", "resnet18", "--protocol", "sfmlearner"], "monodepth2"),
            (["--pretrained-posenet", str(ckpt), "--pose-model", "resnet18"], "FOLDER"),
            (["--pretrained-posenet", str(folder), "--pose-model", "posecnn"], "FILE"),
            (["--pretrained-posenet", str(ckpt), "--batch", "0"], "--batch"),
            (["--pretrained-posenet", str(ckpt), "--sequences"], "--sequences")):
        with pytest.raises(SystemExit) as e:
            eval_pose.parse_args(argv)
        assert word in str(e.value), (argv, str(e.value))
    args = eval_pose.parse_args(["--pretrained-posenet", str(ckpt)])
    assert (args.pose_model, args.protocol, args.batch, args.sequences, args.img_height, args.img_width) == ("poseexp", "sfmlearner", 32, ["09"], 128, 416)
    assert eval_pose.parse_args(["--pretrained-posenet", str(folder), "--pose-model", "resnet18", "--readers", "99"]).readers == PE.MAX_READERS
    assert eval_pose.parse_args(["--pretrained-posenet", str(ckpt), "--pose-model", "posecnn"]).protocol == "monodepth2"


def test_help_lists_every_flag_of_the_readme():
    text = eval_pose.build_parser().format_help()
    readme = open(os.path.join(ROOT, "README.md")).read()
    flags = ("--pretrained-posenet", "--pose-model", "--protocol", "--dataset-dir", "--sequences", "--dataset-format", "--img-height",
             "--img-width", "--no-resize", "--rotation-mode", "--img-exts", "--batch", "--readers", "--host-chain", "--output-dir", "--dump-poses")
    for f in flags:
        assert f in text, f
    lines = [l for l in readme.splitlines() if "eval_pose.py" in l and l.strip().startswith("python")]
    assert lines, "README.md has no eval_pose.py command line"
    for l in lines:
        for word in l.replace("\\", " ").split():
            if word.startswith("--"):
                assert word in flags, word


def test_predictions_shapes():
    pose, gt, mode = A.sfm_case("well", 2, 5)
    F = PE.predictions("sfmlearner", pose, mode)
    assert F.shape == (2, 5, 3, 4) and np.array_equal(F[0], PE.sfm_final_poses(pose[0], mode))
    assert np.allclose(F[:, 0, :, :3] @ np.transpose(F[:, 0, :, :3], (0, 2, 1)), np.eye(3))
    m, _ = A.mono2_case("well", 3)
    assert PE.predictions("monodepth2", m).shape == (3, 4, 4)
