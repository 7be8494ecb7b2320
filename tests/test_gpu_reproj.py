"""The monodepth2 self-supervision kernels (csrc/dn_reproj.hip) on the GPU: the pose / geometry layers, the fused minimum-reprojection
loss and networks.PoseCNN against the fp64 restatement of tests/reproj_audit.py, the exact cases, and one training step eagerly and
on a launch tape.  pytest -m gpu.

Every tolerance is geom_audit.check(): MARGIN x the fp32 CPU evaluation's own error against fp64 on the same inputs, the fragile
pixels carrying a zero upstream gradient (tests/test_reproj_audit_host.py shows what that rejects).  Each comparison prints its
figures.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import reproj_audit as RA  # noqa: E402
import supervised_dispnet_amd.layers as L  # noqa: E402
import supervised_dispnet_amd.loss_functions as LF  # noqa: E402
import supervised_dispnet_amd.models as models  # noqa: E402
import supervised_dispnet_amd.networks as networks  # noqa: E402
from oracle import detgen  # noqa: E402
from supervised_dispnet_amd.optim import FusedAdam  # noqa: E402
from test_gpu_models import grad_close  # noqa: E402

DEV = torch.device("cuda:0")
F64, F32 = torch.float64, torch.float32


def dev(t):
    return t.to(DEV)


# ---------------------------------------------------------------------------------------------------- pose / geometry layers
@pytest.mark.parametrize("invert", [False, True])
def test_transformation_from_parameters_vs_fp64(invert):
    aa, tr = RA.pose_vectors()
    r64, r32 = RA.pose_reference(invert, F64), RA.pose_reference(invert, F32)
    # the two vectors as views of one [B, 1, 6] tensor, as networks.PoseCNN hands them over: read through their strides
    base = dev(torch.cat([aa, tr], 2))
    a, t = base[..., :3].detach().requires_grad_(), base[..., 3:].detach().requires_grad_()
    assert not a.is_contiguous()
    m = L.transformation_from_parameters(a, t, invert=invert)
    (m * dev(RA.pose_weight())).sum().backward()
    for k, (q, got) in enumerate((("M", m), ("daxisangle", a.grad), ("dtranslation", t.grad))):
        RA.check("transformation:invert%d:%s" % (invert, q), got, r64[k], r32[k])
    # the zero rotation: values only (the norm has no gradient there)
    z = torch.zeros(1, 1, 3, device=DEV)
    t1 = dev(tr[:1])
    m0 = L.transformation_from_parameters(z, t1, invert=invert).cpu()
    want = RA.transformation_from_parameters(torch.zeros(1, 1, 3, dtype=F64), tr[:1].double(), invert)
    assert torch.equal(m0.double(), want.float().double())
    r = L.rot_from_axisangle(dev(aa))
    RA.check("rot_from_axisangle", r, RA.rot_from_axisangle(aa.double()), RA.rot_from_axisangle(aa))
    assert torch.equal(L.get_translation_matrix(dev(tr)).cpu(), RA.get_translation_matrix(tr))


@pytest.mark.parametrize("size", RA.GEOM_SIZES, ids=lambda s: "%dx%d" % s)
def test_backproject_project3d_vs_fp64(size):
    h, w = size
    i = RA.geom_inputs(size)
    r64, r32 = RA.geom_reference(size, F64), RA.geom_reference(size, F32)
    b = i["depth"].shape[0]
    depth = dev(i["depth"]).requires_grad_()
    bp = L.BackprojectDepth(b, h, w)
    assert not list(bp.parameters())
    pts = bp(depth, dev(i["inv_K"]))
    (pts * dev(i["gp"])).sum().backward()
    p, t = dev(r32["points"]).requires_grad_(), dev(i["T"]).requires_grad_()
    grid = L.Project3D(b, h, w)(p, dev(i["K"]), t)
    (grid * dev(i["gg"])).sum().backward()
    tag = "geom:%dx%d:" % size
    RA.check(tag + "points", pts, r64["points"], r32["points"])
    RA.check(tag + "ddepth", depth.grad, r64["ddepth"], r32["ddepth"])
    # Project3D on the fp32 points: its own fp64 / fp32 references on exactly those
    p64, t64 = r32["points"].double().requires_grad_(), i["T"].double().requires_grad_()
    g64, _ = RA.project(p64, i["K"].double(), t64, h, w)
    (g64 * i["gg"].double()).sum().backward()
    p32, t32 = r32["points"].clone().requires_grad_(), i["T"].clone().requires_grad_()
    g32, _ = RA.project(p32, i["K"], t32, h, w)
    (g32 * i["gg"]).sum().backward()
    RA.check(tag + "grid", grid, g64.detach(), g32.detach())
    RA.check(tag + "dpoints", p.grad, p64.grad, p32.grad)
    RA.check(tag + "dT", t.grad, t64.grad, t32.grad)


# ------------------------------------------------------------------------------------------------------------- the fused loss
def _gpu_loss(name, align, automask, ties=True):
    i = RA.inputs(name)
    disp = dev(i["disp"]).requires_grad_()
    T = [dev(t).requires_grad_() for t in i["T"]]
    args = (dev(i["tgt"]), [dev(r) for r in i["refs"]], disp, dev(i["K"]), dev(i["inv_K"]), T)
    kw = dict(min_depth=RA.MIN_DEPTH, max_depth=RA.MAX_DEPTH, automask=automask, ssim_weight=RA.SSIM_W, align_corners=align)
    m = LF.min_reprojection_loss(*args, reduction="none", **kw)
    sel = m._dn_selection
    (m * dev(RA.upstream(name, align, automask, ties))).sum().backward()
    with torch.no_grad():
        loss = LF.min_reprojection_loss(*args, reduction="mean", **kw)
    torch.cuda.synchronize()
    return dict(m=m.detach(), loss=loss, sel=sel, ddisp=disp.grad, dT=[t.grad for t in T])


@pytest.mark.parametrize("automask", RA.AUTOMASKS, ids=["automask", "plain"])
@pytest.mark.parametrize("align", RA.ALIGNS, ids=["ac0", "ac1"])
@pytest.mark.parametrize("name", RA.LOSS_CASES)
def test_min_reprojection_loss_vs_fp64(name, align, automask):
    r64, r32 = RA.reference(name, align, automask, F64), RA.reference(name, align, automask, F32)
    got = _gpu_loss(name, align, automask)
    tag = "%s:ac%d:am%d:" % (name, align, automask)
    RA.check(tag + "m", got["m"], r64["m"], r32["m"])
    RA.check(tag + "loss", got["loss"], r64["loss"], r32["loss"])
    off_tie = ~r64["near_tie"]
    assert torch.equal(got["sel"].cpu().long()[off_tie], r64["sel"][off_tie]), tag + "selection map"
    assert got["sel"].dtype == torch.uint8
    RA.check(tag + "ddisp", got["ddisp"], r64["ddisp"], r32["ddisp"])
    for f, g in enumerate(got["dT"]):
        RA.check(tag + "dT%d" % f, g, r64["dT"][f], r32["dT"][f])


def test_identical_frames_give_exactly_zero():
    i = RA.inputs("select_ragged")
    tgt = dev(i["tgt"])
    disp = dev(i["disp"]).requires_grad_()
    T = [dev(t).requires_grad_() for t in i["T"]]
    loss = LF.min_reprojection_loss(tgt, [tgt, tgt], disp, dev(i["K"]), dev(i["inv_K"]), T)
    loss.backward()
    assert float(loss.detach()) == 0.0
    assert int(loss._dn_selection.max()) == 0
    assert float(disp.grad.abs().max()) == 0.0 and all(float(t.grad.abs().max()) == 0.0 for t in T)


@pytest.mark.parametrize("automask", RA.AUTOMASKS, ids=["automask", "plain"])
def test_twin_frames_select_the_lower_index(automask):
    """two identical source frames under identical T: every tie goes to the lower channel, which alone takes the gradient"""
    name = "twins"
    r64, r32 = RA.reference(name, False, automask, F64, False), RA.reference(name, False, automask, F32, False)
    got = _gpu_loss(name, False, automask, ties=False)
    sel = got["sel"].cpu().long()
    nf = RA.CASES[name]["F"]
    assert bool(((sel == 0) | (sel == (nf if automask else 0))).all()) and torch.equal(sel, r64["sel"])
    assert float(got["dT"][1].abs().max()) == 0.0
    RA.check("twins:am%d:ddisp" % automask, got["ddisp"], r64["ddisp"], r32["ddisp"])
    RA.check("twins:am%d:dT0" % automask, got["dT"][0], r64["dT"][0], r32["dT"][0])


def test_two_calls_are_bitwise_equal():
    a, b = _gpu_loss("seams", False, True), _gpu_loss("seams", False, True)
    for k in ("m", "loss", "sel", "ddisp"):
        assert torch.equal(a[k], b[k]), k
    for x, y in zip(a["dT"], b["dT"]):
        assert torch.equal(x, y)


def test_pose_form_equals_the_matrix_form():
    """T = (axisangle, translation, invert_flags): through the layers when the views carry no base, through the base when they do"""
    name = "select_ragged"
    i = RA.inputs(name)
    up = dev(RA.upstream(name, False, True))
    common = (dev(i["tgt"]), [dev(r) for r in i["refs"]])
    a, t = dev(i["axisangle"]).requires_grad_(), dev(i["translation"]).requires_grad_()
    d1 = dev(i["disp"]).requires_grad_()
    m1 = LF.min_reprojection_loss(*common, d1, dev(i["K"]), dev(i["inv_K"]), (a, t, list(i["invert"])), reduction="none")
    (m1 * up).sum().backward()
    base = dev(torch.cat([i["axisangle"], i["translation"]], 3)).requires_grad_()          # [B, F, 1, 6]
    va, vt = base[..., :3], base[..., 3:]
    va._dn_pose_base = vt._dn_pose_base = base
    d2 = dev(i["disp"]).requires_grad_()
    m2 = LF.min_reprojection_loss(*common, d2, dev(i["K"]), dev(i["inv_K"]), (va, vt, list(i["invert"])), reduction="none")
    (m2 * up).sum().backward()
    assert torch.equal(m1, m2) and torch.equal(d1.grad, d2.grad)
    # the same dT through the same Rodrigues backward, once inside the loss's pose kernel and once in the layer's own: two fp32
    # compilations of one formula (FMA contraction differs), a few units of round-off of the largest component apart
    for got, want in ((base.grad[..., :3], a.grad), (base.grad[..., 3:], t.grad)):
        assert float(want.abs().max()) > 0
        assert float((got - want).abs().max()) <= 16 * RA.FLOOR * float(want.abs().max())


# ------------------------------------------------------------------------------------------------------------------ PoseCNN
def test_pose_cnn_vs_golden(golden):
    g = golden("reproj")
    net = networks.PoseCNN(2)
    assert list(net.state_dict().keys()) == list(g["posecnn:keys"])
    net.load_state_dict(RA.pose_cnn_state())
    torch_layout = torch.nn.ModuleDict({"net": torch.nn.ModuleList([torch.nn.Conv2d(*a) for a in (
        (6, 16, 7, 2, 3), (16, 32, 5, 2, 2), (32, 64, 3, 2, 1), (64, 128, 3, 2, 1), (128, 256, 3, 2, 1), (256, 256, 3, 2, 1), (256, 256, 3, 2, 1))]),
        "pose_conv": torch.nn.Conv2d(256, 6, 1)})
    torch_layout.load_state_dict(net.state_dict())                     # strict: the keys and shapes of torch's own module layout
    net.to(DEV).train()
    aa, tr = net(dev(RA.pose_cnn_input()))
    assert tuple(aa.shape) == tuple(tr.shape) == (2, 1, 1, 3)
    ga, gt = RA.pose_cnn_weights()
    ((aa * dev(ga)).sum() + (tr * dev(gt)).sum()).backward()
    a64, t64, g64 = RA.pose_cnn_reference(F64)
    a32, t32, g32 = RA.pose_cnn_reference(F32)
    for q, got, want in (("axisangle", aa, g["posecnn:axisangle"]), ("translation", tr, g["posecnn:translation"])):
        got, want = got.detach().cpu(), torch.as_tensor(want)
        assert float((got - want).abs().max()) <= 1e-3 * float(want.abs().max()) + 1e-7, q
    RA.check("posecnn:axisangle", aa, a64, a32)
    RA.check("posecnn:translation", tr, t64, t32)
    params = dict(net.named_parameters())
    for k in RA.POSE_CNN_KEYS:
        grad_close("posecnn:grad:" + k, params[k].grad, g64[k])


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


def test_training_step_eager_and_taped():
    from supervised_dispnet_amd.graph import TapedStep, backward
    depth_net, pose_net, opt, K, Kinv, batch = _step_setup()
    tgt, ref, pair = (t.clone() for t in batch(0))

    def step():
        disp = depth_net(tgt)[0]
        axisangle, translation = pose_net(pair)
        loss = LF.min_reprojection_loss(tgt, [ref], disp, K, Kinv, (axisangle, translation, [False]))
        opt.zero_grad()
        backward(loss)
        opt.step()
        return loss

    p0 = opt.arena.flat_p.clone()
    l0 = step()                                                    # eagerly
    torch.cuda.synchronize()
    assert torch.isfinite(l0) and float(l0) > 0
    moved, still = {"pose": 0, "depth": 0}, []
    for net, which in ((pose_net, "pose"), (depth_net, "depth")):          # parameters and Adam moments of BOTH networks moved
        offs = {id(p): o for p, o in zip(opt.arena.params, opt.arena.offsets)}
        names = {id(p): n for n, p in net.named_parameters()}
        for p in net._hot_parameters():
            name = names[id(p)]
            sl = slice(offs[id(p)], offs[id(p)] + p.numel())
            if float((opt.arena.flat_p[sl] - p0[sl]).abs().max()) > 0:
                assert float(opt.exp_avg[sl].abs().max()) > 0 and float(opt.exp_avg_sq[sl].abs().max()) > 0, name
                moved[which] += 1
            else:
                still.append(which + ":" + name)
    print("moved", moved, "unmoved", still)
    # the loss reads the finest disparity only: the three coarser heads (weight and bias each) are the only parameters it cannot reach
    assert moved["pose"] == len(RA.POSE_CNN_KEYS) and len(still) <= 6 and all(s.startswith("depth:decoder") for s in still), still
    ts = TapedStep(step, optimizer=opt, warmup=1, static_inputs=(tgt, ref, pair)).capture()
    assert ts.launches > 100 and ts.segments == 1
    for dst, src in zip((tgt, ref, pair), batch(1)):               # a second batch: framework-side work the tape missed would read stale data
        dst.copy_(src)
    state = opt.tape_state() + [b for b in depth_net.buffers() if b.is_cuda]
    same, worst = ts.verify(state)
    assert same, "the replayed step differs from the eager one by %.3g" % worst
    ts.close()
