"""monodepth2's multi-scale objective (csrc/dn_mono2.hip, loss_functions.monodepth2_loss) on the GPU against the fp64 restatement of
tests/mono2_audit.py, the exact cases, a training step eagerly and on a launch tape, and train.py --min-reprojection.  pytest -m gpu.

Every tolerance is mono2_audit.check() (= geom_audit's): MARGIN x the fp32 CPU evaluation's own error against fp64 on the same inputs;
the gradients are those of the objective whose per-pixel minimum carries the case's upstream map, zero on the fragile pixels of each
scale.  Each comparison prints its figures.
"""
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
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import mono2_audit as MA  # noqa: E402
import reproj_audit as RA  # noqa: E402
import supervised_dispnet_amd.loss_functions as LF  # noqa: E402
import supervised_dispnet_amd.models as models  # noqa: E402
import supervised_dispnet_amd.networks as networks  # noqa: E402
from oracle import detgen  # noqa: E402
from supervised_dispnet_amd.optim import FusedAdam  # noqa: E402

DEV = torch.device("cuda:0")
F64, F32 = torch.float64, torch.float32
KW = dict(min_depth=RA.MIN_DEPTH, max_depth=RA.MAX_DEPTH, ssim_weight=RA.SSIM_W)


def dev(t):
    return t.to(DEV)


def _gpu(name, align, automask, S=MA.S_MAX, smoothness=MA.SMOOTHNESS, refs=None, weighted=True):
    """values of the plain objective, gradients of the weighted one (mono2_audit.weights)"""
    i = MA.inputs(name)
    disps = [dev(d).requires_grad_() for d in i["disps"][:S]]
    T = [dev(t).requires_grad_() for t in i["T"]]
    refs = [dev(r) for r in i["refs"]] if refs is None else refs
    args = (dev(i["tgt"]), refs, disps, dev(i["K"]), dev(i["inv_K"]), T)
    kw = dict(KW, automask=automask, smoothness=smoothness, align_corners=align)
    with torch.no_grad():
        val = LF.monodepth2_loss(*args, **kw)
    w = dev(MA.weights(name, align, automask, S)) if weighted else None
    loss = LF.monodepth2_loss(*args, _pixel_weights=w, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return dict(loss=val.detach(), parts=val._dn_parts, sel=val._dn_selection, ddisp=[d.grad for d in disps], dT=[t.grad for t in T])


@pytest.mark.parametrize("automask", MA.AUTOMASKS, ids=["automask", "plain"])
@pytest.mark.parametrize("align", MA.ALIGNS, ids=["ac0", "ac1"])
@pytest.mark.parametrize("name", MA.FULL_CASES + MA.VALUE_CASES)
def test_monodepth2_loss_vs_fp64(name, align, automask):
    r64, r32 = MA.reference(name, align, automask, F64), MA.reference(name, align, automask, F32)
    got = _gpu(name, align, automask)
    tag = "%s:ac%d:am%d:" % (name, align, automask)
    assert got["loss"].dim() == 0 and got["loss"].is_cuda and tuple(got["parts"].shape) == (MA.S_MAX, 2) and got["parts"].is_cuda
    MA.check(tag + "loss", got["loss"], r64["loss"], r32["loss"])
    MA.check(tag + "parts:reprojection", got["parts"][:, 0], r64["parts"][:, 0], r32["parts"][:, 0])
    MA.check(tag + "parts:smoothness", got["parts"][:, 1], r64["parts"][:, 1], r32["parts"][:, 1])
    for s in range(MA.S_MAX):
        MA.check(tag + "ddisp%d" % s, got["ddisp"][s], r64["ddisp"][s], r32["ddisp"][s])
    if name in MA.VALUE_CASES:
        assert all(float(g.abs().max()) == 0.0 for g in got["dT"])          # no reprojection gradient was asked for
        return
    for s in range(MA.S_MAX):
        off_tie = ~r64["near_tie"][s]
        assert got["sel"][s].dtype == torch.uint8
        assert torch.equal(got["sel"][s].cpu().long()[off_tie], r64["sel"][s][off_tie]), tag + "selection map of scale %d" % s
    for f, g in enumerate(got["dT"]):
        MA.check(tag + "dT%d" % f, g, r64["dT"][f], r32["dT"][f])


def test_one_scale_without_smoothness_is_min_reprojection_loss_bit_for_bit():
    name = "ms_seams"
    i = MA.inputs(name)
    for automask in MA.AUTOMASKS:
        d1, d2 = dev(i["disps"][0]).requires_grad_(), dev(i["disps"][0]).requires_grad_()
        T1, T2 = [dev(t).requires_grad_() for t in i["T"]], [dev(t).requires_grad_() for t in i["T"]]
        common = (dev(i["tgt"]), [dev(r) for r in i["refs"]])
        a = LF.monodepth2_loss(*common, [d1], dev(i["K"]), dev(i["inv_K"]), T1, smoothness=0.0, scaled_disp=False, automask=automask, **KW)
        b = LF.min_reprojection_loss(*common, d2, dev(i["K"]), dev(i["inv_K"]), T2, automask=automask, **KW)
        a.backward()
        b.backward()
        assert torch.equal(a.detach(), b.detach()) and torch.equal(a._dn_selection[0], b._dn_selection)
        assert torch.equal(d1.grad, d2.grad)
        for x, y in zip(T1, T2):
            assert torch.equal(x.grad, y.grad)


def test_identical_frames_give_exactly_zero():
    i = MA.inputs("ms_select")
    tgt = dev(i["tgt"])
    got = _gpu("ms_select", False, True, smoothness=0.0, refs=[tgt, tgt], weighted=False)
    assert float(got["parts"][:, 0].abs().max()) == 0.0 and float(got["loss"]) == 0.0
    assert all(int(s.max()) == 0 for s in got["sel"])
    assert all(float(g.abs().max()) == 0.0 for g in got["ddisp"]) and all(float(g.abs().max()) == 0.0 for g in got["dT"])
    # with the smoothness on, the reprojection parts stay exactly 0 and the gradient is the smoothness gradient alone
    got = _gpu("ms_select", False, True, refs=[tgt, tgt], weighted=False)
    assert float(got["parts"][:, 0].abs().max()) == 0.0 and float(got["parts"][:, 1].min()) > 0.0
    assert all(float(g.abs().max()) == 0.0 for g in got["dT"]) and all(float(g.abs().max()) > 0.0 for g in got["ddisp"])


def test_two_calls_are_bitwise_equal():
    a, b = _gpu("ms_seams", False, True), _gpu("ms_seams", False, True)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["parts"], b["parts"])
    for k in ("sel", "ddisp", "dT"):
        for x, y in zip(a[k], b[k]):
            assert torch.equal(x, y), k


def test_scaled_disp_is_the_reciprocal():
    """scaled_disp=True: depth = 1 / up.  The same depths reach the kernel as disp_to_depth(up') for up' = (up - 1/max) / (1/min - 1/max)
    only approximately, so compare against the restatement with depth = 1 / up instead."""
    i = MA.inputs("ms_select")
    c = lambda t, dt: t.to(dt)
    scaled = [d * 40 for d in i["disps"][:2]]                               # fp32 inputs: depths of 1 / (40 disp), around 1
    outs = {}
    for dt in (F64, F32):
        tgt, refs = c(i["tgt"], dt), [c(r, dt) for r in i["refs"]]
        total = 0
        for s in range(2):
            d = c(scaled[s], dt)
            up = MA.upsample(d, tgt.shape[2:])
            lo, span = 1 / RA.MAX_DEPTH, 1 / RA.MIN_DEPTH - 1 / RA.MAX_DEPTH
            ev = RA.evaluate(tgt, refs, (up - lo) / span, c(i["K"], dt), c(i["inv_K"], dt), [c(t, dt) for t in i["T"]], False, True)
            total = total + ev["m"].mean()
        outs[dt] = total / 2
    got = LF.monodepth2_loss(dev(i["tgt"]), [dev(r) for r in i["refs"]], [dev(d) for d in scaled], dev(i["K"]), dev(i["inv_K"]),
                             [dev(t) for t in i["T"]], scaled_disp=True, smoothness=0.0, ssim_weight=RA.SSIM_W)
    MA.check("scaled_disp:loss", got, outs[F64], outs[F32])


def test_bad_shapes_raise():
    i = MA.inputs("ms_select")
    args = lambda disps, tgt=i["tgt"]: (dev(tgt), [dev(r) for r in i["refs"]], disps, dev(i["K"]), dev(i["inv_K"]), [dev(t) for t in i["T"]])
    d = [dev(x) for x in i["disps"]]
    with pytest.raises(ValueError):
        LF.monodepth2_loss(*args([]))
    with pytest.raises(ValueError):
        LF.monodepth2_loss(*args(d + [d[3]]))
    with pytest.raises(ValueError):
        LF.monodepth2_loss(*args([d[0], d[2]]))
    j = RA.inputs("select_ragged")                                          # 23 x 37: not divisible by 2
    with pytest.raises(ValueError):
        LF.monodepth2_loss(dev(j["tgt"]), [dev(r) for r in j["refs"]], [dev(j["disp"]), dev(j["disp"])[:, :, :11, :18]], dev(j["K"]),
                           dev(j["inv_K"]), [dev(t) for t in j["T"]])


def _pose_run(name, pose):
    i = MA.inputs(name)
    disps = [dev(d).requires_grad_() for d in i["disps"]]
    w = dev(MA.weights(name, False, True))
    loss = LF.monodepth2_loss(dev(i["tgt"]), [dev(r) for r in i["refs"]], disps, dev(i["K"]), dev(i["inv_K"]), pose, smoothness=MA.SMOOTHNESS,
                              _pixel_weights=w, **KW)
    loss.backward()
    return loss.detach(), [d.grad for d in disps]


def test_pose_form_equals_the_matrix_form():
    """T = (axisangle, translation, invert_flags): through the layers when the views carry no base; through the base when they do, in
    PoseCNN's batch-major layout and in the frame-major layout train.py --min-reprojection hands over"""
    name = "ms_select"
    i = MA.inputs(name)
    flags = list(i["invert"])
    a, t = dev(i["axisangle"]).requires_grad_(), dev(i["translation"]).requires_grad_()
    l1, g1 = _pose_run(name, (a, t, flags))
    both = torch.cat([i["axisangle"], i["translation"]], 3)                                  # [B, F, 1, 6]
    b, f = both.shape[:2]
    base_bm = dev(both.reshape(b, f * 6, 1, 1).contiguous()).requires_grad_()               # PoseCNN's [B, 6 F, 1, 1]
    v = base_bm.view(b, f, 1, 6)
    base_fm = dev(both.permute(1, 0, 2, 3).reshape(f * b, 6, 1, 1).contiguous()).requires_grad_()       # frame-major [F B, 6, 1, 1]
    u = base_fm.view(f, b, 1, 6).permute(1, 0, 2, 3)
    for base, view, back in ((base_bm, v, lambda g: g.view(b, f, 1, 6)), (base_fm, u, lambda g: g.view(f, b, 1, 6).permute(1, 0, 2, 3))):
        va, vt = view[..., :3], view[..., 3:]
        va._dn_pose_base = vt._dn_pose_base = base
        l2, g2 = _pose_run(name, (va, vt, flags))
        assert torch.equal(l1, l2) and all(torch.equal(x, y) for x, y in zip(g1, g2))
        gb = back(base.grad)
        for got, want in ((gb[..., :3], a.grad), (gb[..., 3:], t.grad)):
            assert float(want.abs().max()) > 0
            assert float((got - want).abs().max()) <= 16 * RA.FLOOR * float(want.abs().max())


# ------------------------------------------------------------------------------------------------------------ a training step
def _step_setup():
    b, h, w = 2, 64, 96
    enc = networks.ResnetEncoder(18, False)
    depth_net = models.monodepth2(enc, networks.DepthDecoder(enc.num_ch_enc))
    detgen.fill_state_dict(depth_net.state_dict(), "reproj:step:depth")
    pose_net = networks.PoseCNN(2)
    pose_net.load_state_dict(RA.pose_cnn_state(tag="reproj:step:pose"))
    depth_net.to(DEV).train()
    pose_net.to(DEV).train()
    opt = FusedAdam(list(pose_net._hot_parameters()) + list(depth_net._hot_parameters()), lr=1e-4)
    k, kinv = RA.intrinsics(b, h, w)

    def batch(seed):
        tgt = RA.pattern(b, h, w, "reproj:step:tgt%d" % seed).float()
        ref = (RA.pattern(b, h, w, "reproj:step:tgt%d" % seed, (1.2, 0.4)) + 0.05 * (RA.pattern(b, h, w, "reproj:step:p%d" % seed) - 0.5)).float()
        return dev(tgt), dev(ref), dev(torch.cat([tgt, ref], 1))

    return depth_net, pose_net, opt, dev(k), dev(kinv), batch


def test_training_step_moves_every_parameter_eagerly_and_taped():
    from supervised_dispnet_amd.graph import TapedStep, backward
    depth_net, pose_net, opt, K, Kinv, batch = _step_setup()
    tgt, ref, pair = (t.clone() for t in batch(0))

    def step():
        disps = depth_net(tgt)
        axisangle, translation = pose_net(pair)
        loss = LF.monodepth2_loss(tgt, [ref], disps, K, Kinv, (axisangle, translation, [False]), scaled_disp=True)
        opt.zero_grad()
        backward(loss)
        opt.step()
        return loss

    p0 = opt.arena.flat_p.clone()
    l0 = step()                                                    # eagerly
    torch.cuda.synchronize()
    assert torch.isfinite(l0) and float(l0.detach()) > 0
    still, n = [], 0
    offs = {id(p): o for p, o in zip(opt.arena.params, opt.arena.offsets)}
    for net, which in ((pose_net, "pose"), (depth_net, "depth")):
        names = {id(p): nm for nm, p in net.named_parameters()}
        for p in net._hot_parameters():
            sl = slice(offs[id(p)], offs[id(p)] + p.numel())
            n += 1
            if not float((opt.arena.flat_p[sl] - p0[sl]).abs().max()) > 0:
                still.append(which + ":" + names[id(p)])
    assert n > len(RA.POSE_CNN_KEYS) + 6 and not still, still      # EVERY hot parameter: the three coarser heads included
    ts = TapedStep(step, optimizer=opt, warmup=1, static_inputs=(tgt, ref, pair)).capture()
    assert ts.launches > 100 and ts.segments == 1
    for dst, src in zip((tgt, ref, pair), batch(1)):               # a second batch: framework-side work the tape missed would read stale data
        dst.copy_(src)
    state = opt.tape_state() + [b for b in depth_net.buffers() if b.is_cuda]
    same, worst = ts.verify(state)
    assert same, "the replayed step differs from the eager one by %.3g" % worst
    ts.close()


def test_launch_count_does_not_depend_on_the_number_of_scales():
    """the launches of one forward + backward, counted by the library's launch tape (recorded only, never replayed: no TapedStep, no
    stream or memory pool of its own)"""
    from supervised_dispnet_amd import _lib
    from supervised_dispnet_amd.graph import backward
    lib = _lib.load()
    i = MA.inputs("ms_select")
    common = (dev(i["tgt"]), [dev(r) for r in i["refs"]])
    K, Kinv = dev(i["K"]), dev(i["inv_K"])
    counts = {}
    for S in (1, MA.S_MAX):
        disps = [dev(d).requires_grad_() for d in i["disps"][:S]]
        T = [dev(t).requires_grad_() for t in i["T"]]

        def step():
            for t in disps + T:
                t.grad = None
            backward(LF.monodepth2_loss(*common, disps, K, Kinv, T, **KW))
            torch.cuda.synchronize()

        step()
        tape = lib.dn_tape_begin()
        assert tape, _lib.last_error()
        try:
            step()
            assert lib.dn_tape_end(tape) == 0
            counts[S] = lib.dn_tape_launches(tape)
        finally:
            lib.dn_tape_free(tape)
    f = len(i["refs"])
    print("launches", counts)
    # forward: F identity + F warped + select + means + smoothness + finalize; backward: 2 F + pose + the gather into the coarse maps
    assert counts[1] == counts[MA.S_MAX] == 4 * f + 6


# -------------------------------------------------------------------------------------------------------------- command line
def test_train_cli_min_reprojection(tmp_path):
    """train.py --min-reprojection as a command line of its own (a fresh process: its DataLoader workers, its optimizer arena and
    whatever else a training run sets up stay out of the test process)."""
    import subprocess
    import numpy as np
    from tests.cases import make_scene_folders
    root = make_scene_folders(pathlib.Path(tmp_path) / "kitti", frames=5, h=64, w=96)
    wdir = tmp_path / "mono2_weights"
    wdir.mkdir()
    enc = networks.ResnetEncoder(18, False)
    torch.save(enc.state_dict(), str(wdir / "encoder.pth"))
    torch.save(networks.DepthDecoder(enc.num_ch_enc).state_dict(), str(wdir / "depth.pth"))
    out = tmp_path / "run"
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), str(root), "--unsupervised", "--monodepth2", "--min-reprojection", "--network",
           "disp_res_18", "--pretrained-disp", str(wdir), "-b", "2", "--epochs", "1", "--epoch-size", "2", "--sequence-length", "3", "-s", "1e-3",
           "--with-gt", "--save-root", str(out), "--print-freq", "100"]
    done = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert done.returncode == 0, done.stdout[-3000:]
    runs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs]
    full = [r for r in runs if r.endswith("progress_log_full.csv")][0]
    rows = [l.split("\t") for l in open(full).read().strip().splitlines()]
    assert len(rows) == 1 + 2
    vals = np.array([[float(v) for v in r] for r in rows[1:]])
    assert np.isfinite(vals).all() and (vals[:, 0] > 0).all() and (vals[:, 3] > 0).all()
    pose_ckpt = [r for r in runs if r.endswith("exp_pose_checkpoint.pth.tar")]
    assert len(pose_ckpt) == 1
    psd = torch.load(pose_ckpt[0], map_location="cpu")["state_dict"]
    assert sorted(psd.keys()) == sorted(RA.POSE_CNN_KEYS)                  # a monodepth2 pose.pth layout
