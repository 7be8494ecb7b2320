"""Host side of monodepth2's ResNet pose network (networks.PoseResnet), no GPU: the state-dict layout against the
reference's (tests/golden/pose_resnet.npz), the audit's restatement against the golden values, the tail's derived bounds against the
reference's own fp32 composition, the two-file checkpoint layout and train.py's arguments."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import pose_net_audit as PA  # noqa: E402

F64, F32 = torch.float64, torch.float32


def _shapes(g, prefix, keys):
    return {k: tuple(int(v) for v in g["%s:shape:%s" % (prefix, k)]) for k in keys}


def test_state_dicts_have_the_reference_layout(golden):
    import supervised_dispnet_amd.networks as networks
    g = golden("pose_resnet")
    net = networks.PoseResnet()
    dsd, esd = net.decoder.state_dict(), net.encoder.state_dict()
    dkeys, ekeys = list(g["dec:keys"]), list(g["enc:keys"])
    assert list(dsd.keys()) == dkeys == PA.DECODER_KEYS                            # a monodepth2 pose.pth
    assert {k: tuple(v.shape) for k, v in dsd.items()} == _shapes(g, "dec", dkeys) == PA.DECODER_SHAPES
    assert list(esd.keys()) == ekeys == list(PA.encoder_state().keys())            # a monodepth2 pose_encoder.pth
    assert {k: tuple(v.shape) for k, v in esd.items()} == _shapes(g, "enc", ekeys)
    assert tuple(esd["encoder.conv1.weight"].shape) == (64, 6, 7, 7)
    hot = {id(p) for p in net._hot_parameters()}
    names = {id(p): n for n, p in net.named_parameters()}
    assert sorted(names[i] for i in set(names) - hot) == ["encoder.encoder.fc.bias", "encoder.encoder.fc.weight"]
    assert len(hot) == len(net._hot_parameters())


def test_audit_restatement_reproduces_the_golden(golden):
    g = golden("pose_resnet")
    aa, tr, grads = PA.decoder_reference(F32)
    for q, got in (("axisangle", aa), ("translation", tr)):
        want = torch.as_tensor(g["dec:" + q])
        assert tuple(got.shape) == tuple(want.shape) == (2, 2, 1, 3)
        assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max()) + 1e-9, q
    for k in PA.DECODER_KEYS:
        want = g["dec:grad:%s:samples" % k]
        got = grads[k].double().reshape(-1).numpy()[::PA.grad_stride(grads[k].numel())]
        assert np.abs(got - want).max() <= 1e-3 * np.abs(want).max() + 1e-12, k
        assert abs(float(grads[k].double().abs().sum()) - float(g["dec:grad:%s:abssum" % k])) <= 1e-3 * float(g["dec:grad:%s:abssum" % k]), k
    # the loss reads the first transform only: the second half of pose_2 gets no gradient in the reference either
    assert float(grads["net.3.weight"][6:].abs().max()) == 0 and float(grads["net.3.bias"][6:].abs().max()) == 0
    assert float(grads["net.3.weight"][:6].abs().max()) > 0
    # the whole network, train-mode BatchNorm
    aa, tr, feat, _, _ = PA.net_reference(F32)
    want = g["enc:last:samples"]
    got = feat.double().reshape(-1).numpy()[::53]
    assert tuple(feat.shape) == tuple(int(v) for v in g["enc:last:shape"]) == PA.DEC_FEATURE
    assert np.abs(got - want).max() <= 1e-3 * np.abs(want).max() + 1e-9
    for q, got in (("axisangle", aa), ("translation", tr)):
        want = torch.as_tensor(g["net:" + q])
        assert float((got - want).abs().max()) <= 1e-3 * float(want.abs().max()) + 1e-7, q


@pytest.mark.parametrize("case", PA.TAIL_CASES, ids=lambda c: "P%d-HW%d-C%d-O%d-used%d" % c)
def test_fp32_composed_tail_keeps_the_derived_bounds(case):
    """The bounds are ones plain fp32 torch on the CPU keeps -- not ones fitted to the kernel.  Mean first (the order the operation
    counts are derived for): all four bounds as stated.  Conv first, as the reference composes the tail: out, dx and dw as stated; its
    bias gradient is a sum of P * HW per-pixel terms `scale * dout / HW`, not of P, so the P + 1 operations of the stated bound do not
    describe it (measured at P 3, HW 52: 1.87 x that bound) and it is held to its own count, P * HW + 2.  The kernel is held to P + 1
    (tests/test_gpu_pose_net.py)."""
    i = PA.tail_inputs(*case)
    P, HW = case[0], case[1]
    PA.tail_check("mean-first fp32 %s" % (case,), PA.tail_composed(i, F32, mean_first=True), i)
    got = PA.tail_composed(i, F32)
    PA.tail_check("conv-first fp32 %s" % (case,), got, i, dbias_ops=P * HW + 2)
    if case[3] > case[4]:
        assert float(got["dw"][case[4]:].abs().max()) == 0 and float(got["dbias"][case[4]:].abs().max()) == 0


def test_tail_bounds_are_not_vacuous():
    """a 1 % error of a typical element is outside them"""
    i = PA.tail_inputs(3, 52, 256, 12, 6)
    ref = PA.tail_composed(i, F64)
    for k in ("out", "dx", "dw", "dbias"):
        b, r = PA.tail_bounds(i)[k], ref[k]
        live = r != 0
        assert float((b[live] / r[live].abs()).median()) < 1e-2, k


def _filled_net():
    import supervised_dispnet_amd.networks as networks
    net = networks.PoseResnet()
    net.encoder.load_state_dict(PA.encoder_state())
    net.decoder.load_state_dict(PA.decoder_state())
    return net


def test_monodepth2_folder_round_trip(tmp_path):
    import supervised_dispnet_amd.networks as networks
    net = _filled_net()
    folder = str(tmp_path / "mono_640x192")
    net.save_monodepth2(folder)
    assert sorted(os.listdir(folder)) == ["pose.pth", "pose_encoder.pth"]
    pose = torch.load(os.path.join(folder, "pose.pth"))
    assert list(pose.keys()) == PA.DECODER_KEYS and tuple(pose["net.0.weight"].shape) == (256, 512, 1, 1)       # bare state dicts
    assert list(torch.load(os.path.join(folder, "pose_encoder.pth")).keys()) == list(PA.encoder_state().keys())
    fresh = networks.PoseResnet()
    fresh.load_monodepth2(folder)
    for (k, a), (_, b) in zip(net.state_dict().items(), fresh.state_dict().items()):
        assert torch.equal(a, b), k
    # a pose_encoder.pth without the unused classifier loads too; any other missing key is refused by name
    enc = {k: v for k, v in net.encoder.state_dict().items() if ".fc." not in k}
    torch.save(enc, os.path.join(folder, "pose_encoder.pth"))
    networks.PoseResnet().load_monodepth2(folder)
    del enc["encoder.layer3.0.downsample.0.weight"]
    torch.save(enc, os.path.join(folder, "pose_encoder.pth"))
    with pytest.raises(RuntimeError, match=r"encoder\.layer3\.0\.downsample\.0\.weight"):
        networks.PoseResnet().load_monodepth2(folder)


def test_a_posecnn_pose_pth_is_refused_by_name(tmp_path):
    import supervised_dispnet_amd.networks as networks
    folder = str(tmp_path / "posecnn")
    _filled_net().save_monodepth2(folder)
    torch.save(networks.PoseCNN(2).state_dict(), os.path.join(folder, "pose.pth"))
    with pytest.raises(RuntimeError, match=r"net\.0\.weight.*\[16, 6, 7, 7\]"):
        networks.PoseResnet().load_monodepth2(folder)
    with pytest.raises(RuntimeError, match="FOLDER"):
        networks.PoseResnet().load_monodepth2(os.path.join(folder, "pose.pth"))


def test_train_arguments(tmp_path):
    import train
    p = train.build_parser()
    base = ["DATA", "--unsupervised", "--monodepth2", "--network", "disp_res_18"]
    assert p.parse_args(["DATA"]).pose_model == "posecnn"
    train.check_dataset_args(p.parse_args(base + ["--min-reprojection"]))
    train.check_dataset_args(p.parse_args(base + ["--min-reprojection", "--pose-model", "resnet18"]))
    with pytest.raises(SystemExit, match="--min-reprojection"):
        train.check_dataset_args(p.parse_args(base + ["--pose-model", "resnet18"]))
    f = tmp_path / "pose.pth"
    f.write_bytes(b"")
    with pytest.raises(SystemExit, match="FOLDER.*a file"):
        train.check_dataset_args(p.parse_args(base + ["--min-reprojection", "--pose-model", "resnet18", "--pretrained-exppose", str(f)]))
    train.check_dataset_args(p.parse_args(base + ["--min-reprojection", "--pose-model", "resnet18", "--pretrained-exppose", str(tmp_path)]))
    train.check_dataset_args(p.parse_args(base + ["--min-reprojection", "--pretrained-exppose", str(f)]))       # PoseCNN: a file, as before
    with pytest.raises(SystemExit):
        p.parse_args(["DATA", "--pose-model", "resnet50"])
    assert "depth network only" in " ".join(p.format_help().split())


def test_pose_decoder_still_raises():
    import supervised_dispnet_amd.networks as networks
    with pytest.raises(NotImplementedError, match="PoseResnet"):
        networks.PoseDecoder()
