"""Disp_vgg_BN at the NYU Depth v2 shapes of `train.py --dataset nyu --with-gt`, every convolution call checked against fp64.

Kernel selection depends on the grid, not only on the layer (tile shapes by block count, K / pixel splits, the 8-wave Winograd
kernel and its tail split), and the NYU grids are not KITTI's: b32 x 256 x 352 for training (and its per-rank shards b16 / b8 / b4),
eval mode at 320 x 448 with a ragged last batch for validation (654 test images: 14 = 654 mod 32, 7 = its 2-rank half).

  * training / validation audit (tests/conv_audit.py): every forward, input-gradient and weight-gradient call of one real step, on
    the data the network produced, against an fp64 evaluation of the call's contract, |got - ref| <= c u A per element (+ relative
    L2 <= 5e-6); the fused BatchNorm statistics / BatchNorm-backward sums / bias gradients / reciprocals against fp64 sums of the
    kernels' own outputs; every hot convolution seen exactly once per pass.  KITTI's metric shape b32 x 128 x 416 is one more
    parameter.
  * dispatch census: an unaudited step of the same shape with per-launch profiling on lists the kernels the shape selects; the audit
    must have covered every one of them.  The census is printed per shape.
  * network parity with the CPU oracle at b32 x 256 x 352 (training: loss, disparities, gradients, running statistics -- the
    tolerances of test_gpu_metric_shape.py) and eval-mode disp0 at 320 x 448.
"""
import os
import sys

import numpy as np
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
from oracle import detgen, losses as OL, nets as ON  # noqa: E402
from supervised_dispnet_amd import engine  # noqa: E402
from supervised_dispnet_amd.functional import reciprocal  # noqa: E402
from test_gpu_metric_shape import VGG_GRAD_KEYS  # noqa: E402
from test_gpu_models import _is_pre_bn_conv_bias, _oracle_params, close, grad_close  # noqa: E402

DEV = torch.device("cuda:0")

# (id, batch, height, width, compute mode, dataset)
TRAIN_SHAPES = [("nyu_b32_f32x3", 32, 256, 352, "f32x3", "nyu"), ("nyu_b32_f32", 32, 256, 352, "f32", "nyu"),
                ("nyu_b16_f32x3", 16, 256, 352, "f32x3", "nyu"), ("nyu_b8_f32x3", 8, 256, 352, "f32x3", "nyu"),
                ("nyu_b4_f32x3", 4, 256, 352, "f32x3", "nyu"), ("kitti_b32_f32x3", 32, 128, 416, "f32x3", "kitti")]
EVAL_SHAPES = [("nyu_eval_b32", 32, 320, 448), ("nyu_eval_b14", 14, 320, 448), ("nyu_eval_b7", 7, 320, 448)]
CENSUS = {}
WORST = {}


def _net(datasets):
    net = models.Disp_vgg_BN(datasets=datasets, with_classifier=False)
    detgen.fill_state_dict(net.state_dict(), "vggbn")
    return net


def _inputs(tag, B, H, W, datasets):
    x = detgen.image_batch(B, H, W, tag + ":x")
    if datasets == "nyu":
        gt = detgen.sparse_depth(B, H, W, tag + ":gt", density=0.95, lo=0.5, hi=10.0)      # dense-ish indoor depth, max 10 m
    else:
        gt = detgen.sparse_depth(B, H, W, tag + ":gt", density=0.05)
    return x, gt


def _step(net, x, gt, datasets, training):
    if training:
        disps = net(x)
        loss = LF.l1_loss(gt, [reciprocal(d) for d in disps], datasets)
        loss.backward()
    else:
        with torch.no_grad():
            net(x)
    torch.cuda.synchronize()


def _census(monkeypatch, net, x, gt, datasets, training):
    """Kernels one unaudited step selects for its convolution calls (engine.PROFILE's per-launch records)."""
    rec = []
    monkeypatch.setattr(engine, "PROFILE", rec)
    try:
        _step(net, x, gt, datasets, training)
    finally:
        monkeypatch.setattr(engine, "PROFILE", None)
    return sorted({r[0] for r in rec if r[4].split(" ")[0] in ("conv_fwd", "convT_fwd", "conv_dgrad", "convT_dgrad", "conv_wgrad",
                                                               "convT_wgrad")})


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
    CENSUS[tag] = census


def _audit_run(monkeypatch, tag, net, x, gt, datasets, training):
    census = _census(monkeypatch, net, x, gt, datasets, training)
    net.zero_grad(set_to_none=True)
    with monkeypatch.context() as mp:
        au = CA.audit(mp, net)
        _step(net, x, gt, datasets, training)
        au.flush()
    _report(tag, au, census)
    cover = au.coverage(training)
    assert not cover, "%s: calls not audited exactly once (pass -> {layer: calls}): %s" % (tag, cover)
    missing = set(census) - set(au.kernels())
    assert not missing, "%s: kernels the shape selects that the audit never saw: %s" % (tag, sorted(missing))
    assert not au.failures, "%s: %d checks over the bound:\n%s" % (tag, len(au.failures), "\n".join(
        "%s %s %s %s err/(uA) %.3g (c %s) relL2 %.3g, %d over" % (r["layer"], r["pass"], r["kernel"], r["what"], r["worst"], r["c"],
                                                                  r["rel"], r["over"]) for r in au.failures))


@pytest.mark.parametrize("shape", TRAIN_SHAPES, ids=[s[0] for s in TRAIN_SHAPES])
def test_training_step_every_conv_call_vs_fp64(monkeypatch, shape):
    tag, B, H, W, mode, datasets = shape
    x, gt = _inputs(tag, B, H, W, datasets)
    prev = engine.compute_mode()
    engine.set_compute(mode)
    try:
        net = _net(datasets).to(DEV).train()
        _audit_run(monkeypatch, tag, net, x.to(DEV), gt.to(DEV), datasets, True)
    finally:
        engine.set_compute(prev)


@pytest.mark.parametrize("shape", EVAL_SHAPES, ids=[s[0] for s in EVAL_SHAPES])
def test_validation_forward_every_conv_call_vs_fp64(monkeypatch, shape):
    tag, B, H, W = shape
    x, _ = _inputs(tag, B, H, W, "nyu")
    net = _net("nyu").to(DEV).eval()
    _audit_run(monkeypatch, tag + "_f32x3", net, x.to(DEV), None, "nyu", False)


def test_census_and_worst_errors_summary():
    """Prints what the audits above found (the census per shape and the worst err / (u A) per kernel family and mode); every audit
    that ran left a census."""
    assert all(CENSUS.values())
    print("\n== dispatch census per shape")
    for tag, ks in CENSUS.items():
        print("%s: %s" % (tag, ", ".join(ks)))
    print("== worst err / (u A) per kernel family, pass, mode")
    for (fam, pas, mode), w in sorted(WORST.items()):
        print("%-12s %-6s %-6s %.3g (c %s)" % (fam, pas, mode, w, "32 + log2(P), x 2 Winograd" if pas == "wgrad" else CA.bound(
            "dn::wino_conv" if fam == "wino" else "dn::igemm", pas)))


# --------------------------------------------------------------------------------------------------- network parity vs oracle
B, H, W = 32, 256, 352
EH, EW, EB = 320, 448, 14
_ORACLE = {}


def _nyu_oracle():
    if "train" not in _ORACLE:
        net = _net("nyu")
        sd0 = {k: v.clone() for k, v in net.state_dict().items()}
        x, gt = _inputs("nyu32", B, H, W, "nyu")
        osd = _oracle_params(sd0)
        with CA.capped_threads():
            odisps = ON.disp_vgg_bn(osd, x, training=True, datasets="nyu")
            oloss = OL.l1_loss(gt, [1 / d for d in odisps], "nyu")
            oloss.backward()
        _ORACLE["train"] = (sd0, x, gt, [d.detach() for d in odisps], float(oloss.item()),
                            {k: v.grad.clone() for k, v in osd.items() if getattr(v, "grad", None) is not None},
                            {k: v.detach().clone() for k, v in osd.items() if "running" in k})
    return _ORACLE["train"]


@pytest.mark.parametrize("mode", ["f32x3", "f32"])
def test_disp_vgg_bn_nyu_at_32x256x352_vs_oracle(mode):
    sd0, x, gt, odisps, oloss, ograds, obn = _nyu_oracle()
    prev = engine.compute_mode()
    engine.set_compute(mode)
    try:
        net = models.Disp_vgg_BN(datasets="nyu", with_classifier=False)
        net.load_state_dict(sd0)
        net.to(DEV).train()
        disps = net(x.to(DEV))
        loss = LF.l1_loss(gt.to(DEV), [reciprocal(d) for d in disps], "nyu")
        loss.backward()
        torch.cuda.synchronize()
    finally:
        engine.set_compute(prev)
    np.testing.assert_allclose(loss.item(), oloss, rtol=1e-4)
    for i, (d, od) in enumerate(zip(disps, odisps)):
        assert tuple(d.shape) == tuple(od.shape)
        got, want = d.detach().reshape(-1)[::97].cpu(), od.reshape(-1)[::97]
        close("%s disp%d[::97]" % (mode, i), got, want, rtol=1e-3, atol_rel=1e-4)
        np.testing.assert_allclose(float(d.double().sum()), float(od.double().sum()), rtol=1e-4)
    named = dict(net.named_parameters())
    for key in VGG_GRAD_KEYS:
        grad_close("%s grad:%s" % (mode, key), named[key].grad, ograds[key])
    for name, p in named.items():
        if _is_pre_bn_conv_bias(name):
            assert float(p.grad.abs().max()) == 0.0
        elif name in ograds:
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
    sd1 = net.state_dict()
    for key in ("features.features.1.running_mean", "features.features.1.running_var", "features.features.41.running_mean",
                "features.features.41.running_var"):
        close(mode + " " + key, sd1[key], obn[key], rtol=1e-3, atol_rel=1e-4)


def test_disp_vgg_bn_nyu_eval_at_320x448_vs_oracle():
    """Validation's forward (eval mode, running statistics) on the ragged last batch of the 654-image test split."""
    net = _net("nyu")
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    x, _ = _inputs("nyu_eval14", EB, EH, EW, "nyu")
    with CA.capped_threads(), torch.no_grad():
        od = ON.disp_vgg_bn(_oracle_params(sd0), x, training=False, datasets="nyu")
    net.to(DEV).eval()
    with torch.no_grad():
        d = net(x.to(DEV))
    torch.cuda.synchronize()
    assert tuple(d.shape) == tuple(od.shape) == (EB, 1, EH, EW)
    close("eval disp0[::97]", d.reshape(-1)[::97].cpu(), od.reshape(-1)[::97], rtol=1e-3, atol_rel=1e-4)
    np.testing.assert_allclose(float(d.double().sum()), float(od.double().sum()), rtol=1e-4)
