"""Frozen BatchNorm through whole networks on the GPU (pytest -m gpu): net.train() followed by bn.eval() on some or all BatchNorm
modules must behave as in PyTorch -- the frozen modules normalise with their running statistics, move no buffer, and their backward
(one pass per layer, csrc/dn_bn.hip dn_bn_frozen_*) yields the gradients of the same network evaluated by the CPU oracle.

Reference: the oracle's own networks (oracle/nets*.py), whose one BatchNorm statement `_bn(sd, prefix, x, training)` is wrapped for the
duration of a test so that the modules named frozen run with training=False while the network keeps its training outputs.  The running
statistics are randomised (mean 0.3 * randn, variance in [0.5, 2]) so that frozen and batch statistics differ: each test first checks,
on the CPU, that the oracle's frozen output differs from its training-mode output by far more than the forward tolerance -- a path
that wrongly used batch statistics cannot pass.

Tolerances are those tests/test_gpu_models.py applies to the same networks: forward rtol 1e-3 / atol 1e-4 max|ref| (Disp_vgg_BN),
rtol 2e-3 / atol 2e-4 max|ref| (the ResNet / FCRN nets); every parameter gradient -- the conv biases in front of a frozen BatchNorm
included, which are no longer zero -- relative L2 <= 2e-2, <= 1 % outliers, scale within 3e-3 (grad_close, copied from there)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import supervised_dispnet_amd.loss_functions as LF  # noqa: E402
import supervised_dispnet_amd.models as models  # noqa: E402
from oracle import detgen, losses as OL, nets as ON, nets_res as ONR, nets_zoo as ONZ  # noqa: E402  (the checker)
from supervised_dispnet_amd.functional import reciprocal  # noqa: E402
from supervised_dispnet_amd.optim import FusedAdam  # noqa: E402

DEV = torch.device("cuda:0")


def close(name, got, want, rtol, atol_rel):
    got = got.detach().float().cpu()
    want = torch.as_tensor(want).detach().float().cpu()
    assert got.shape == want.shape, "%s: shape %s vs %s" % (name, tuple(got.shape), tuple(want.shape))
    scale = float(want.abs().max()) + 1e-30
    err = (got - want).abs()
    tol = atol_rel * scale + rtol * want.abs()
    bad = err > tol
    if bad.any():
        idx = np.unravel_index(int(torch.argmax(err - tol)), got.shape)
        raise AssertionError("%s: %d/%d off; worst at %s got %.7g want %.7g (max|want| %.4g, max err %.4g)" % (
            name, int(bad.sum()), got.numel(), idx, float(got[idx]), float(want[idx]), scale, float(err.max())))


def grad_close(name, got, want, rtol=1e-2, atol_rel=1e-2, max_bad_frac=1e-2, max_rel_l2=2e-2, max_scale_dev=3e-3):
    """Flip-robust gradient comparison of tests/test_gpu_models.py (see its module docstring), same thresholds."""
    got = got.detach().double().cpu()
    want = torch.as_tensor(want).detach().double().cpu()
    assert got.shape == want.shape, "%s: shape %s vs %s" % (name, tuple(got.shape), tuple(want.shape))
    assert torch.isfinite(got).all(), "%s: non-finite gradient" % name
    scale = float(want.abs().max()) + 1e-30
    err = (got - want).abs()
    nbad = int((err > atol_rel * scale + rtol * want.abs()).sum())
    bad = nbad / got.numel()
    rel_l2 = float(err.norm() / (want.norm() + 1e-30))
    assert (bad <= max_bad_frac or nbad <= 2) and rel_l2 <= max_rel_l2, "%s: %.3g%% elements off, relative L2 error %.3g (max err %.3g of max|ref| %.3g)" % (
        name, 100 * bad, rel_l2, float(err.max()), scale)
    wn = float((want * want).sum())
    if wn > 0 and got.numel() >= 8:
        c = float((got * want).sum()) / wn
        assert abs(c - 1.0) <= max_scale_dev, "%s: gradient scale <got,want>/<want,want> = %.6f (|c-1| > %.1g); relative L2 %.3g" % (
            name, c, max_scale_dev, rel_l2)


def _is_bn(m):
    return m.__class__.__name__.find("BatchNorm") != -1


def _fresh(net, prefix):
    """Closed-form parameters, then running statistics that differ from any batch's: mean 0.3 * randn, variance in [0.5, 2]."""
    detgen.fill_state_dict(net.state_dict(), prefix)
    gen = torch.Generator().manual_seed(1234)
    for k, v in net.state_dict().items():
        if k.endswith("running_mean"):
            v.copy_(0.3 * torch.randn(v.shape, generator=gen))
        elif k.endswith("running_var"):
            v.copy_(0.5 + 1.5 * torch.rand(v.shape, generator=gen))
    return {k: v.clone() for k, v in net.state_dict().items()}


def _oracle_params(sd, dtype=torch.float32):
    out = {}
    for k, v in sd.items():
        v = v.detach().cpu().clone()
        if torch.is_floating_point(v):
            v = v.to(dtype)
            if "running" not in k:
                v.requires_grad_(True)
        out[k] = v
    return out


def _freeze_oracle(monkeypatch, frozen):
    """`frozen(prefix)`: the oracle's BatchNorm at that state_dict prefix runs with training=False, whatever the network's flag."""
    orig = ON._bn

    def bn(sd, p, x, training):
        return orig(sd, p, x, training and not frozen(p))

    for mod in (ON, ONR, ONZ):
        monkeypatch.setattr(mod, "_bn", bn)


def _freeze_modules(net, frozen):
    names = []
    for name, m in net.named_modules():
        if _is_bn(m) and frozen(name):
            m.eval()
            names.append(name)
    return names


def _loss(lf, gt, outs, ds, recip):
    depth = [recip(d) for d in outs]
    return lf.l1_loss(gt, depth, ds) + 0.1 * lf.smooth_loss(depth)


def _run_case(monkeypatch, net, tag, run, ds, frozen, rtol, atol_rel, shape=(2, 64, 96), net_training=True, extra=None, skip=()):
    """One step of `net` with the BatchNorms selected by `frozen` in eval mode against the oracle; returns (net, names of frozen modules)."""
    b, h, w = shape
    sd0 = _fresh(net, "frozen:" + tag)
    net.to(DEV).train(net_training)
    names = _freeze_modules(net, frozen) if net_training else [n for n, m in net.named_modules() if _is_bn(m)]
    assert names, "nothing frozen"
    x = detgen.image_batch(b, h, w, "frozen:%s:x" % tag)
    gt = detgen.sparse_depth(b, h, w, "frozen:%s:gt" % tag, density=0.6, lo=0.3, hi=11.0)
    # ---- the oracle: frozen as asked, and (on a copy) with every BatchNorm on batch statistics
    _freeze_oracle(monkeypatch, frozen if net_training else (lambda p: True))
    osd = _oracle_params(sd0)
    oouts = run(osd, x, net_training)
    oouts = list(oouts) if isinstance(oouts, (tuple, list)) else [oouts]
    _loss(OL, gt, oouts, ds, lambda d: 1 / d).backward()
    monkeypatch.undo()
    with torch.no_grad():
        touts = run(_oracle_params(sd0), x, True)
    touts = list(touts) if isinstance(touts, (tuple, list)) else [touts]
    gap = float((oouts[0].detach() - touts[0]).abs().max())
    tol = (atol_rel + rtol) * float(oouts[0].detach().abs().max())
    assert gap > 20 * tol, "%s: frozen and batch statistics agree to %.3g (forward tolerance %.3g): the case shows nothing" % (tag, gap, tol)
    # ---- the HIP path
    if extra is not None:
        extra(net)
    outs = net(x.to(DEV))
    outs = list(outs) if isinstance(outs, (tuple, list)) else [outs]
    assert len(outs) == len(oouts)
    _loss(LF, gt.to(DEV), outs, ds, reciprocal).backward()
    torch.cuda.synchronize()
    for i, (d, od) in enumerate(zip(outs, oouts)):
        close("%s:disp%d" % (tag, i), d, od, rtol=rtol, atol_rel=atol_rel)
    checked = 0
    for name, p in net.named_parameters():
        if name in skip or ".classifier." in name or ".fc." in name:
            continue
        og = osd[name].grad
        if og is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None, name
        grad_close("%s grad:%s" % (tag, name), p.grad, og)
        checked += 1
    assert checked > 10
    # ---- buffers: bit-identical where frozen, moved elsewhere
    sd1 = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    for name, m in net.named_modules():
        if not _is_bn(m):
            continue
        keys = [name + s for s in (".running_mean", ".running_var", ".num_batches_tracked")]
        same = [torch.equal(sd1[k], sd0[k]) for k in keys]
        if name in names:
            assert all(same), "%s: a buffer of the frozen %s moved" % (tag, name)
        elif name not in skip:
            assert not any(same), "%s: %s trains but a buffer of it did not move" % (tag, name)
    return net, names, osd


def _pre_bn_conv_biases_are_live(net, osd, keys):
    for k in keys:
        g = dict(net.named_parameters())[k].grad
        assert float(osd[k].grad.abs().max()) > 0 and float(g.abs().max()) > 0, k


def test_disp_vgg_bn_all_frozen(monkeypatch):
    """The pool form (the last BatchNorm of each stage) and the ReLU form (the others); 13 conv biases in front of a frozen BatchNorm."""
    net = models.Disp_vgg_BN(datasets="kitti", with_classifier=False)
    net, names, osd = _run_case(monkeypatch, net, "vggbn", lambda sd, x, tr: ON.disp_vgg_bn(sd, x, training=tr), "kitti", lambda p: True,
                                rtol=1e-3, atol_rel=1e-4)
    assert len(names) == 13
    _pre_bn_conv_biases_are_live(net, osd, ["features.features.0.bias", "features.features.40.bias"])


def test_disp_vgg_bn_eval_mode_backward(monkeypatch):
    """net.eval() followed by a backward: the same path, one output."""
    net = models.Disp_vgg_BN(datasets="kitti", with_classifier=False)
    _run_case(monkeypatch, net, "vggbn_eval", lambda sd, x, tr: ON.disp_vgg_bn(sd, x, training=tr), "kitti", lambda p: True,
              rtol=1e-3, atol_rel=1e-4, net_training=False)


def test_disp_res_50_all_frozen(monkeypatch):
    """The residual tail with a frozen downsample branch and with an identity branch; the discarded bn1 moves nothing when frozen."""
    net = models.Disp_res_50(datasets="nyu")
    net, names, _ = _run_case(monkeypatch, net, "res50", lambda sd, x, tr: ONR.disp_res_50(sd, x, training=tr, datasets="nyu"), "nyu",
                              lambda p: True, rtol=2e-3, atol_rel=2e-4, skip=("bn1.weight", "bn1.bias"))
    assert "bn1" in names and "layer1.0.downsample.1" in names
    assert net.bn1.weight.grad is None and net.bn1.bias.grad is None


def test_disp_res_18_mixed(monkeypatch):
    """layer1 and layer2 frozen, the rest on batch statistics: a training producer under a frozen consumer (stem -> layer1) and a
    frozen producer under a training consumer (layer2 -> layer3), i.e. the input-gradient kernels' fused BatchNorm sums on both sides
    of the boundary."""
    from tests.cases import zoo_cases
    _, cls, kwargs, ds, run = [c for c in zoo_cases() if c[0] == "res18"][0]
    net = getattr(models, cls)(**kwargs)
    frozen = lambda p: p.startswith("layer1.") or p.startswith("layer2.")
    net, names, _ = _run_case(monkeypatch, net, "res18", run, ds, frozen, rtol=2e-3, atol_rel=2e-4, skip=("bn1.weight", "bn1.bias"))
    assert "layer2.0.downsample.1" in names and not any(n.startswith("layer3") for n in names)


def test_fcrn_all_frozen(monkeypatch):
    """block_bn_plain (bn2) and block_upproject (BatchNorm over the interleaved maps, conv biases in front of them)."""
    from tests.cases import zoo2_cases, zoo2_dropout_mask
    _, cls, kwargs, run = [c for c in zoo2_cases() if c[0] == "fcrn"][0]
    mask = zoo2_dropout_mask("fcrn")
    net = getattr(models, cls)(**kwargs)

    def extra(n):
        n._dropout_mask = mask

    net, names, osd = _run_case(monkeypatch, net, "fcrn", lambda sd, x, tr: run(sd, x, tr, mask), "kitti", lambda p: True, rtol=2e-3,
                                atol_rel=2e-4, extra=extra)
    assert "bn2" in names and "up1.bn1_2" in names
    _pre_bn_conv_biases_are_live(net, osd, ["up1.conv1_1.bias", "up4.conv3.bias"])


def test_mixed_modes_within_one_residual_tail_are_refused():
    net = models.Disp_res_18(datasets="nyu")
    detgen.fill_state_dict(net.state_dict(), "frozen:res18")
    net.to(DEV).train()
    net.layer2[0].downsample[1].eval()
    with pytest.raises(RuntimeError, match="both be frozen"):
        net(detgen.image_batch(2, 64, 96, "frozen:refuse:x").to(DEV))


def test_launch_tape_of_a_frozen_step_is_bitwise_the_eager_step():
    """graph.TapedStep of a frozen Disp_vgg_BN step with FusedAdam: the call train.py's TapedTrainer makes -- record on one batch,
    verify() on a second one."""
    from supervised_dispnet_amd.graph import TapedStep, backward
    net = models.Disp_vgg_BN(datasets="kitti", with_classifier=False)
    _fresh(net, "frozen:tape")
    net.to(DEV).train()
    _freeze_modules(net, lambda p: True)
    opt = FusedAdam(net._hot_parameters(), lr=1e-4, production_order=net._grad_production_order())
    b, h, w = 2, 64, 96
    batches = [(detgen.image_batch(b, h, w, "frozen:tape:x%d" % i).to(DEV),
                detgen.sparse_depth(b, h, w, "frozen:tape:gt%d" % i, density=0.3).to(DEV)) for i in range(2)]
    img, gt = batches[0][0].clone(), batches[0][1].clone()
    buffers0 = [t.clone() for t in net.buffers()]

    def step():
        depth = [reciprocal(d) for d in net(img)]
        loss = LF.l1_loss(gt, depth, "kitti")
        opt.zero_grad()
        backward(loss)
        opt.step()
        return loss

    ts = TapedStep(step, optimizer=opt, warmup=0, static_inputs=(img, gt))
    try:
        first = ts()
        assert bool(torch.isfinite(first).all()) and ts.launches > 100
        img.copy_(batches[1][0])
        gt.copy_(batches[1][1])
        same, worst = ts.verify(opt.tape_state() + [t for t in net.buffers() if t.is_cuda])
        assert same, "replay differs from the eager step, max |diff| %.3g" % worst
        torch.cuda.synchronize()
        assert all(torch.equal(a, t) for a, t in zip(buffers0, net.buffers()))
        bias = net.features.features[0].bias
        assert float(opt.arena.flat_g.abs().max()) > 0 and float(bias._dn_grad_view.abs().max()) > 0
    finally:
        ts.close()


def test_train_cli_freeze_bn(tmp_path, capsys):
    """train.py --freeze-bn through the command line, on the launch tape (the default): exits, reports the verified replay, and the
    checkpoint carries the BatchNorm buffers of the start (a fresh network: 0 / 1 / 0)."""
    import train
    train.main(["SYN", "--synthetic", "8", "-b", "2", "--freeze-bn", "--epochs", "1", "--network", "disp_vgg_BN", "--loss", "L1", "--with-gt",
                "--img-height", "64", "--img-width", "96", "--lr", "1e-3", "--save-root", str(tmp_path), "--print-freq", "100"])
    out = capsys.readouterr().out
    assert "--freeze-bn without --pretrained-disp" in out
    assert "launches + " in out and "bit for bit" in out
    runs = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path) for f in fs]
    ckpt = [r for r in runs if r.endswith("dispnet_checkpoint.pth.tar")]
    assert len(ckpt) == 1
    sd = torch.load(ckpt[0], map_location="cpu")["state_dict"]
    seen = 0
    for k, v in sd.items():
        if k.endswith("running_mean"):
            assert float(v.abs().max()) == 0.0, k
            seen += 1
        elif k.endswith("running_var"):
            assert bool((v == 1).all()), k
        elif k.endswith("num_batches_tracked"):
            assert int(v) == 0, k
    assert seen == 13
    full = [r for r in runs if r.endswith("progress_log_full.csv")][0]
    vals = [float(l.split("\t")[0]) for l in open(full).read().strip().splitlines()[1:]]
    assert len(vals) == 4 and all(np.isfinite(vals))
