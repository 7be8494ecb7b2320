"""monodepth2's ResNet pose network on the GPU (networks.PoseResnet, csrc/dn_posetail.hip): the fused tail against
fp64 within the DERIVED bounds of tests/pose_net_audit.py, the whole network against the reference's golden and the fp64 restatement, one
training step eagerly and on a launch tape, and train.py --pose-model resnet18 as a command line.  pytest -m gpu.

The tail's shapes are the smallest at which it can go wrong: one pixel; an odd pixel count below a wavefront; the two map sizes of
training (4 x 13, 6 x 20); 130 pairs (more than any chunk a reduction over the pairs could be cut into, and more blocks than one round);
the narrowest and the widest channel count (one and eight float4 lanes per 16, a different thread layout each); each with 6, 12 and 18
rows of which 6 are used.
"""
import ctypes as C
import os
import pathlib
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import geom_audit as GA  # noqa: E402
import pose_net_audit as PA  # noqa: E402
import reproj_audit as RA  # noqa: E402
import supervised_dispnet_amd.loss_functions as LF  # noqa: E402
import supervised_dispnet_amd.models as models  # noqa: E402
import supervised_dispnet_amd.networks as networks  # noqa: E402
from oracle import detgen  # noqa: E402
from supervised_dispnet_amd import _lib  # noqa: E402
from supervised_dispnet_amd.optim import FusedAdam  # noqa: E402
from test_gpu_models import grad_close  # noqa: E402

DEV = torch.device("cuda:0")
F64, F32 = torch.float64, torch.float32
BAD_ARG = -1


def dev(t):
    return t.to(DEV)


@pytest.fixture(scope="module", autouse=True)
def stream_pool_turn():
    """torch.cuda.Stream() hands out a pool of streams per device round-robin, and tests later in the suite depend on the slot their
    step's stream lands on (a TapedStep on a weight-gradient side stream does not replay the eager step).  The tape
    of this module draws streams; the tests behind it shall find the slot they would have found without it.  Before: one whole turn of
    the pool (the handles in order; ends one slot past where it began).  After: draw until the slot in front of the first one has been
    handed out, so that the next draw is again the first.  Yields the turn."""
    turn, seen = [], set()
    while True:
        h = torch.cuda.Stream(device=DEV).cuda_stream
        if h in seen:
            break
        turn.append(h)
        seen.add(h)
    assert h == turn[0] and 2 <= len(turn) <= 64, (len(turn), "the stream pool is not a round-robin turn")
    yield turn
    for _ in range(len(turn)):
        if torch.cuda.Stream(device=DEV).cuda_stream == turn[-1]:
            break
    else:
        raise AssertionError("the stream pool did not come round to the slot this module started from")


def _next_stream_is_no_side_stream(turn):
    """draw from the pool until the NEXT stream it hands out (the one a TapedStep made now takes) is none of the engine's weight-gradient
    side streams"""
    from supervised_dispnet_amd import engine
    sides = engine.side_stream()["handles"]
    for _ in range(len(turn)):
        h = torch.cuda.Stream(device=DEV).cuda_stream
        if turn[(turn.index(h) + 1) % len(turn)] not in sides:
            return
    raise AssertionError("every pooled stream is a side stream")


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------------ the tail
def _run_tail(i, O):
    """dn_pose_tail_fwd + dn_pose_tail_bwd on the audit inputs -> results shaped like PA.tail_composed's"""
    x = dev(i["x"].float().permute(0, 2, 3, 1).contiguous())                    # [P, HW, 1, C] NHWC
    P, HW, _, Cn = x.shape
    w, b, dout, ou = dev(i["w"].float()), dev(i["b"].float()), dev(i["dout"].float()), i["O_used"]
    mean = torch.empty(P, Cn, device=DEV)
    out = torch.empty(P, ou, device=DEV)
    dx, dw, db = torch.full_like(x, float("nan")), torch.full_like(w, float("nan")), torch.full_like(b, float("nan"))
    _lib.call("dn_pose_tail_fwd", x.data_ptr(), w.data_ptr(), b.data_ptr(), P, HW, Cn, O, ou, i["scale"], mean.data_ptr(), out.data_ptr(),
              _stream())
    _lib.call("dn_pose_tail_bwd", dout.data_ptr(), mean.data_ptr(), w.data_ptr(), P, HW, Cn, O, ou, i["scale"], dx.data_ptr(), dw.data_ptr(),
              db.data_ptr(), _stream())
    torch.cuda.synchronize()
    return dict(out=out, dx=dx.permute(0, 3, 1, 2), dw=dw, dbias=db)


@pytest.mark.parametrize("case", PA.TAIL_CASES, ids=lambda c: "P%d-HW%d-C%d-O%d-used%d" % c)
def test_tail_vs_fp64_within_the_derived_bounds(case):
    P, HW, Cn, O, ou = case
    i = PA.tail_inputs(*case)
    got = _run_tail(i, O)
    PA.tail_check("dn_pose_tail %s" % (case,), got, i)
    if O > ou:                                                                  # the rows the trainer never reads: exact zeros
        assert float(got["dw"][ou:].abs().max()) == 0 and float(got["dbias"][ou:].abs().max()) == 0
    again = _run_tail(i, O)                                                     # fixed summation orders, no atomics
    for k in got:
        assert torch.equal(got[k], again[k]), k


def test_tail_refuses_bad_arguments_without_launching():
    lib = _lib.load()
    buf = torch.zeros(1 << 16, device=DEV)
    p = buf.data_ptr()
    tape = lib.dn_tape_begin()
    assert tape, _lib.last_error()
    try:
        for Cn, O, ou in ((96, 12, 6), (256, 6, 7), (256, 25, 6), (576, 12, 6), (256, 12, 0)):
            assert lib.dn_pose_tail_fwd(p, p, p, 2, 4, Cn, O, ou, 0.01, p, p, _stream()) == BAD_ARG, (Cn, O, ou)
            assert b"dn_pose_tail_fwd" in lib.dn_last_error()
            assert lib.dn_pose_tail_bwd(p, p, p, 2, 4, Cn, O, ou, 0.01, p, p, p, _stream()) == BAD_ARG, (Cn, O, ou)
        assert lib.dn_pose_tail_fwd(p, p, p, 0, 4, 256, 12, 6, 0.01, p, p, _stream()) == BAD_ARG
        assert lib.dn_pose_tail_fwd(p, p, p, 2, 0, 256, 12, 6, 0.01, p, p, _stream()) == BAD_ARG
        assert lib.dn_tape_end(tape) == 0
        assert lib.dn_tape_launches(tape) == 0
    finally:
        lib.dn_tape_free(tape)
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0


# ---------------------------------------------------------------------------------------------------------- the whole network
def _filled_net():
    net = networks.PoseResnet()
    net.encoder.load_state_dict(PA.encoder_state())
    net.decoder.load_state_dict(PA.decoder_state())
    return net


def test_pose_resnet_vs_golden_and_fp64(golden):
    g = golden("pose_resnet")
    net = _filled_net().to(DEV).train()
    aa, tr = net(dev(PA.net_input()))
    assert tuple(aa.shape) == tuple(tr.shape) == (2, 1, 1, 3)
    base = aa._dn_pose_base
    assert base is tr._dn_pose_base and tuple(base.shape) == (2, 6, 1, 1) and base.is_contiguous()
    ga, gt = PA.out_weights()
    ((aa * dev(ga)).sum() + (tr * dev(gt)).sum()).backward()
    a64, t64, _, eg64, dg64 = PA.net_reference(F64)
    a32, t32, _, _, _ = PA.net_reference(F32)
    for q, got, want in (("axisangle", aa, g["net:axisangle"]), ("translation", tr, g["net:translation"])):
        got, want = got.detach().cpu(), torch.as_tensor(want)[:, :1]                # the first predicted transform
        print("golden %s: max |diff| %.3g of max |want| %.3g" % (q, float((got - want).abs().max()), float(want.abs().max())))
        assert float((got - want).abs().max()) <= 1e-3 * float(want.abs().max()) + 1e-7, q
    GA.check("poseresnet:axisangle", aa, a64[:, :1], a32[:, :1])
    GA.check("poseresnet:translation", tr, t64[:, :1], t32[:, :1])
    dparams, eparams = dict(net.decoder.named_parameters()), dict(net.encoder.named_parameters())
    for k in PA.DECODER_KEYS:
        grad_close("poseresnet:decoder:grad:" + k, dparams[k].grad, dg64[k])
    assert float(dparams["net.3.weight"].grad[6:].abs().max()) == 0 and float(dparams["net.3.bias"].grad[6:].abs().max()) == 0
    assert len(eg64) == len(net.encoder._hot_parameters())
    for k, want in eg64.items():                                                     # flip-robust: relative L2 <= 2e-2, <= 1 % outliers,
        grad_close("poseresnet:encoder:grad:" + k, eparams[k].grad, want)            # scale coefficient within 3e-3
    assert eparams["encoder.fc.weight"].grad is None


def test_frozen_batchnorm_forward_equals_eval_forward():
    net = _filled_net().to(DEV).train()
    x = dev(PA.net_input())
    net(x)                                                                           # one training forward: the running statistics move
    before = {k: v.clone() for k, v in net.state_dict().items()}
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    assert net.training and net.encoder.training
    aa, tr = net(x)
    ((aa).sum() + (tr).sum()).backward()                                             # and a backward through the frozen BatchNorms runs
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k                                          # nothing of a frozen BatchNorm moves
    frozen = aa._dn_pose_base.detach().clone()
    net.eval()
    with torch.no_grad():
        aa2, _ = net(x)
    assert torch.equal(frozen, aa2._dn_pose_base)
    assert float(frozen.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ a training step
def test_training_step_eagerly_and_taped(stream_pool_turn):
    from supervised_dispnet_amd.graph import TapedStep, backward
    b, h, w = 2, 64, 96
    enc = networks.ResnetEncoder(18, False)
    depth_net = models.monodepth2(enc, networks.DepthDecoder(enc.num_ch_enc))
    detgen.fill_state_dict(depth_net.state_dict(), "poseresnet:step:depth")
    pose_net = _filled_net()
    depth_net.to(DEV).train()
    pose_net.to(DEV).train()
    opt = FusedAdam(list(pose_net._hot_parameters()) + list(depth_net._hot_parameters()), lr=1e-4)
    k, kinv = RA.intrinsics(b, h, w)
    K, Kinv = dev(k), dev(kinv)

    def batch(seed):
        tgt = RA.pattern(b, h, w, "poseresnet:step:tgt%d" % seed).float()
        ref = (RA.pattern(b, h, w, "poseresnet:step:tgt%d" % seed, (1.2, 0.4)) + 0.05 * (RA.pattern(b, h, w, "poseresnet:step:p%d" % seed) - 0.5)).float()
        return dev(tgt), dev(ref), dev(torch.cat([tgt, ref], 1))

    tgt, ref, pair = (t.clone() for t in batch(0))

    def step():
        disps = depth_net(tgt)
        axisangle, translation = pose_net(pair)
        loss = LF.monodepth2_loss(tgt, [ref], disps, K, Kinv, (axisangle, translation, [False]), scaled_disp=True)
        opt.zero_grad()
        backward(loss)
        opt.step()
        return loss

    w3 = pose_net.decoder.net[3]
    tail0 = (w3.weight.detach()[6:].clone(), w3.bias.detach()[6:].clone())
    p0 = opt.arena.flat_p.clone()
    l0 = step()                                                    # eagerly
    torch.cuda.synchronize()
    assert torch.isfinite(l0) and float(l0.detach()) > 0
    offs = {id(p): o for p, o in zip(opt.arena.params, opt.arena.offsets)}
    names = {id(p): nm for nm, p in pose_net.named_parameters()}
    still, n = [], 0
    for p in pose_net._hot_parameters():                           # every hot parameter of the pose network, with its Adam moments
        sl = slice(offs[id(p)], offs[id(p)] + p.numel())
        n += 1
        moved = float((opt.arena.flat_p[sl] - p0[sl]).abs().max()) > 0
        if not (moved and float(opt.exp_avg[sl].abs().max()) > 0 and float(opt.exp_avg_sq[sl].abs().max()) > 0):
            still.append(names[id(p)])
    assert n == 60 + 8 and not still, still                        # ResNet-18 without fc: 20 convs + 20 BatchNorms x 2; 4 convs x 2
    assert torch.equal(w3.weight.detach()[6:], tail0[0]) and torch.equal(w3.bias.detach()[6:], tail0[1])       # the unread transform
    assert not torch.equal(w3.weight.detach()[:6], dev(PA.decoder_state()["net.3.weight"][:6]))
    _next_stream_is_no_side_stream(stream_pool_turn)
    ts = TapedStep(step, optimizer=opt, warmup=1, static_inputs=(tgt, ref, pair)).capture()
    assert ts.launches > 100 and ts.segments == 1
    for dst, src in zip((tgt, ref, pair), batch(1)):               # a second batch: framework-side work the tape missed would read stale data
        dst.copy_(src)
    state = opt.tape_state() + [t for net in (depth_net, pose_net) for t in net.buffers() if t.is_cuda]
    same, worst = ts.verify(state)
    assert same, "the replayed step differs from the eager one by %.3g" % worst
    assert torch.equal(w3.weight.detach()[6:], tail0[0]) and torch.equal(w3.bias.detach()[6:], tail0[1])
    ts.close()


# -------------------------------------------------------------------------------------------------------------- command line
def test_train_cli_pose_model_resnet18(tmp_path):
    """train.py --min-reprojection --pose-model resnet18 --pretrained-exppose DIR as a command line of its own (a fresh process)."""
    import subprocess
    from tests.cases import make_scene_folders
    root = make_scene_folders(pathlib.Path(tmp_path) / "kitti", frames=5, h=64, w=96)
    wdir = tmp_path / "mono2_weights"
    wdir.mkdir()
    enc = networks.ResnetEncoder(18, False)
    torch.save(enc.state_dict(), str(wdir / "encoder.pth"))
    torch.save(networks.DepthDecoder(enc.num_ch_enc).state_dict(), str(wdir / "depth.pth"))
    start = _filled_net()
    start.save_monodepth2(str(wdir))                               # a released model's folder: all four files side by side
    out = tmp_path / "run"
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), str(root), "--unsupervised", "--monodepth2", "--network", "disp_res_18",
           "--min-reprojection", "--pose-model", "resnet18", "--pretrained-exppose", str(wdir), "--pretrained-disp", str(wdir), "-b", "2",
           "--epochs", "1", "--epoch-size", "2", "--sequence-length", "3", "-s", "1e-3", "--with-gt", "--save-root", str(out),
           "--print-freq", "100"]
    done = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert done.returncode == 0, done.stdout[-3000:]
    assert "=> pose model: resnet18 (PoseResnet)" in done.stdout
    folders = [dp for dp, _, fs in os.walk(out) if os.path.basename(dp) == "pose_mono2"]
    assert len(folders) == 1 and sorted(os.listdir(folders[0])) == ["pose.pth", "pose_encoder.pth"]
    ckpt = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f == "exp_pose_checkpoint.pth.tar"]
    assert len(ckpt) == 1
    trained = networks.PoseResnet()
    trained.load_monodepth2(folders[0])                            # a run can be continued from what it wrote
    assert list(torch.load(ckpt[0], map_location="cpu")["state_dict"].keys()) == list(trained.state_dict().keys())
    s0, s1 = start.state_dict(), trained.state_dict()
    changed = [k for k in s0 if torch.is_floating_point(s0[k]) and ".fc." not in k and not torch.equal(s0[k], s1[k])]
    same = [k for k in s0 if torch.is_floating_point(s0[k]) and ".fc." not in k and torch.equal(s0[k], s1[k])]
    assert not same, same                                          # two iterations moved every weight and every running statistic
    assert len(changed) == 20 + 20 * 4 + 8
    assert all(torch.isfinite(v).all() for v in s1.values() if torch.is_floating_point(v))
    assert torch.equal(s0["encoder.encoder.fc.weight"], s1["encoder.encoder.fc.weight"])       # not a hot parameter: never trained
