"""Every convolution call of the other networks bench.py times, at their real shapes, checked against fp64.

tests/test_gpu_nyu_shapes.py audits Disp_vgg_BN at the NYU and KITTI training / validation shapes.  Kernel selection depends on the
grid, not only on the layer (tile shapes by block count, K / pixel splits, the Winograd tail split, thin / lds3k / stemk forms), so
a kernel wrong only on the other configurations' grids would pass there.  Here, one real step per shape:

  * Disp_res_50 (NYU) at b16 x 480 x 640 (BASELINE configs[3], f32x3 and f32), its per-rank batches b8 / b2 at 2 / 8 GPUs, the
    `train.py --network disp_res_50 --dataset nyu --with-gt` shape b32 x 256 x 352 and the ragged validation batch 14 x 320 x 448;
  * monodepth2(ResnetEncoder(50), DepthDecoder) at b16 x 480 x 640: the reflection-padded decoder;
  * Disp_vgg_BN (NYU) at b16 x 480 x 640, the largest grid the bench runs;
  * Disp_vgg_BN_DORN (K = 80, fused ordinal head) at b32 x 128 x 416 (configs[4]): the trunk's convolutions and the fused head
    (probabilities, decoded labels, d(x), and d(W), d(b) reduced over all 1.7 M pixels);
  * Disp_vgg_BN + PoseExpNet (2 references, no explainability) at b32 x 128 x 416 (configs[2]): bench.py's photometric step, both
    nets audited.

Each audit (tests/conv_audit.py) asserts zero checks over the bound, every hot convolution seen exactly once per pass, and every
kernel of the shape's census (an unaudited step with engine.PROFILE on) covered.  The census and the worst err / (u A) per kernel
family, pass and mode are printed.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import conv_audit as CA  # noqa: E402
import supervised_dispnet_amd.loss_functions as LF  # noqa: E402
import supervised_dispnet_amd.models as models  # noqa: E402
import supervised_dispnet_amd.networks as networks  # noqa: E402
import supervised_dispnet_amd.utils as U  # noqa: E402
from oracle import detgen  # noqa: E402
from supervised_dispnet_amd import engine  # noqa: E402
from supervised_dispnet_amd.functional import reciprocal  # noqa: E402

DEV = torch.device("cuda:0")
CONV_OPS = ("conv_fwd", "convT_fwd", "conv_dgrad", "convT_dgrad", "conv_wgrad", "convT_wgrad")
CENSUS = {}
WORST = {}


def _nyu_gt(tag, B, H, W):
    return detgen.sparse_depth(B, H, W, tag + ":gt", density=0.95, lo=0.5, hi=10.0)


def _l1(net, tag, B, H, W, scale01=False, smooth=0.0):
    """(nets, step, exclusions): the NYU L1 loss step of bench.py's vggbn480 / res50_480 (train.py --loss L1); `smooth`: + that
    weight of the smoothness loss over all scales (monodepth2's coarser heads feed nothing else)."""
    x = detgen.image_batch(B, H, W, tag + ":x").to(DEV)
    if scale01:
        x = (x + 1) / 2                                   # monodepth2 nets take [0, 1] images
    gt = _nyu_gt(tag, B, H, W).to(DEV)

    def step(training):
        if training:
            depth = [reciprocal(d) for d in net(x)]
            loss = LF.l1_loss(gt, depth, "nyu")
            (loss + smooth * LF.smooth_loss(depth) if smooth else loss).backward()
        else:
            with torch.no_grad():
                net(x)
    return [net], step, ()


def res50(tag, B, H, W):
    net = models.Disp_res_50(datasets="nyu")
    detgen.fill_state_dict(net.state_dict(), "res50")
    return _l1(net.to(DEV), tag, B, H, W)


def md2_res50(tag, B, H, W):
    enc = networks.ResnetEncoder(50, False)
    net = models.monodepth2(enc, networks.DepthDecoder(enc.num_ch_enc))
    detgen.fill_state_dict(net.state_dict(), "md2")
    return _l1(net.to(DEV), tag, B, H, W, scale01=True, smooth=0.1)      # the loss of test_config4_full_step_16x480x640


def vggbn(tag, B, H, W):
    net = models.Disp_vgg_BN(datasets="nyu", with_classifier=False)
    detgen.fill_state_dict(net.state_dict(), "vggbn")
    return _l1(net.to(DEV), tag, B, H, W)


def dorn(tag, B, H, W):
    """bench.py's dorn128: SID labels of the ground truth + the DORN loss over the fused head's probabilities."""
    net = models.Disp_vgg_BN_DORN(datasets="kitti", ordinal_c=80, with_classifier=False)
    detgen.fill_state_dict(net.state_dict(), "dorn")
    net.to(DEV)
    net._dropout_mask = (detgen.bernoulli((B, 16), tag + ":drop", 0.5).float() * 2.0).to(DEV)
    x = detgen.image_batch(B, H, W, tag + ":x").to(DEV)
    gt = detgen.sparse_depth(B, H, W, tag + ":gt", density=0.05).to(DEV)

    def step(training):
        target = U.get_labels_sid(gt, ordinal_c=80, dataset="kitti")
        _dec, ordc = net(x)
        LF.DORN_loss(gt, ordc, target, "kitti").backward()
    return [net], step, ("conv_ord",)


def photo(tag, B, H, W):
    """bench.py's photo128: photometric reconstruction over 2 references x 4 scales + 0.1 * smoothness, PoseExpNet trained too."""
    net = models.Disp_vgg_BN(datasets="kitti", with_classifier=False)
    detgen.fill_state_dict(net.state_dict(), "vggbn")
    pose_net = models.PoseExpNet(nb_ref_imgs=2, output_exp=False)
    detgen.fill_state_dict(pose_net.state_dict(), "pose")
    net.to(DEV)
    pose_net.to(DEV)
    x = detgen.image_batch(B, H, W, tag + ":x")
    refs = [(x + 0.05 * (detgen.uniform(x.shape, tag + ":ref%d" % i) * 2 - 1)).clamp(-1, 1).to(DEV) for i in range(2)]
    x = x.to(DEV)
    K = torch.tensor([[241.67, 0, 204.17], [0, 246.28, 59.0], [0, 0, 1]], dtype=torch.float32)
    Kb, Kib = K.repeat(B, 1, 1).to(DEV), torch.inverse(K).repeat(B, 1, 1).to(DEV)

    def step(training):
        mask, pose = pose_net(x, refs)
        depth = [reciprocal(d) for d in net(x)]
        l1 = LF.photometric_reconstruction_loss(x, refs, Kb, Kib, depth, mask, pose, "euler", "zeros")
        (l1 + 0.1 * LF.smooth_loss(depth)).backward()
    return [net, pose_net], step, ()


# (id, builder, batch, height, width, compute mode, training)
SHAPES = [("res50_480_b16_f32x3", res50, 16, 480, 640, "f32x3", True), ("res50_480_b16_f32", res50, 16, 480, 640, "f32", True),
          ("res50_480_b8_f32x3", res50, 8, 480, 640, "f32x3", True), ("res50_480_b2_f32x3", res50, 2, 480, 640, "f32x3", True),
          ("res50_nyu_b32_f32x3", res50, 32, 256, 352, "f32x3", True), ("res50_nyu_eval_b14_f32x3", res50, 14, 320, 448, "f32x3", False),
          ("md2_res50_480_b16_f32x3", md2_res50, 16, 480, 640, "f32x3", True), ("vggbn480_b16_f32x3", vggbn, 16, 480, 640, "f32x3", True),
          ("dorn128_b32_f32x3", dorn, 32, 128, 416, "f32x3", True), ("photo128_b32_f32x3", photo, 32, 128, 416, "f32x3", True)]


def _census(monkeypatch, step, training):
    rec = []
    monkeypatch.setattr(engine, "PROFILE", rec)
    try:
        step(training)
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(engine, "PROFILE", None)
    return sorted({r[0] for r in rec if r[4].split(" ")[0] in CONV_OPS})


def _report(tag, au, census):
    print("\n== %s: %d audited checks" % (tag, len(au.rows)))
    print(au.table())
    print("-- census %s:" % tag)
    for k in census:
        print("   " + k)
    for (fam, pas), w in sorted(au.worst_by_family().items()):
        print("-- worst err/(u A) %s %s %s: %.3g" % (tag, fam, pas, w))
        key = (fam, pas, tag.rsplit("_", 1)[-1])
        WORST[key] = max(WORST.get(key, 0.0), w)
    head = [r for r in au.rows if r["kernel"].startswith("dn::ord_head")]
    for r in head:
        print("-- ord head %s %s %s: err/(uA) %.3g (c %s) relL2 %.3g, %d over" % (tag, r["pass"], r["what"], r["worst"], r["c"], r["rel"],
                                                                              r["over"]))
    CENSUS[tag] = census


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_step_every_conv_call_vs_fp64(monkeypatch, shape):
    tag, builder, B, H, W, mode, training = shape
    prev = engine.compute_mode()
    engine.set_compute(mode)
    try:
        nets, step, exclude = builder(tag, B, H, W)
        for n in nets:
            n.train(training)
        census = _census(monkeypatch, step, training)
        for n in nets:
            n.zero_grad(set_to_none=True)
        with monkeypatch.context() as mp:
            au = CA.audit(mp, *nets, exclude=exclude)
            step(training)
            torch.cuda.synchronize()
            au.flush()
    finally:
        engine.set_compute(prev)
    _report(tag, au, census)
    assert census, "%s: the step selected no convolution kernel" % tag
    cover = au.coverage(training)
    assert not cover, "%s: calls not audited exactly once (pass -> {layer: calls}): %s" % (tag, cover)
    missing = set(census) - set(au.kernels())
    assert not missing, "%s: kernels the shape selects that the audit never saw: %s" % (tag, sorted(missing))
    if builder is dorn:
        whats = {r["what"].split("(")[0] for r in au.rows if r["kernel"].startswith("dn::ord_head")}
        assert whats == {"P", "decode", "head_dx", "head_dw", "head_db"}, whats
    assert not au.failures, "%s: %d checks over the bound:\n%s" % (tag, len(au.failures), "\n".join(
        "%s %s %s %s err/(uA) %.3g (c %s) relL2 %.3g, %d over %s" % (r["layer"], r["pass"], r["kernel"], r["what"], r["worst"], r["c"],
                                                                     r["rel"], r["over"], r["geo"]) for r in au.failures))


def test_census_and_worst_errors_summary():
    """Prints what the audits above found (the census per shape and the worst err / (u A) per kernel family and mode); every audit
    that ran left a census."""
    assert all(CENSUS.values())
    print("\n== dispatch census per shape")
    for tag, ks in CENSUS.items():
        print("%s: %s" % (tag, ", ".join(ks)))
    print("== worst err / (u A) per kernel family, pass, mode")
    for (fam, pas, mode), w in sorted(WORST.items()):
        c = "32 + log2(P)%s" % (", x 2" if fam == "wino_wgrad" else "") if pas == "wgrad" else CA.bound(
            {"wino": "dn::wino_conv", "ord_head": "dn::ord_head"}.get(fam, "dn::igemm"), pas)
        print("%-12s %-6s %-6s %.3g (c %s)" % (fam, pas, mode, w, c))
