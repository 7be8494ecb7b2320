"""optim.FusedSGD / dn_sgd_step on the GPU: torch.optim.SGD's arithmetic (momentum, weight decay, dampening 0, nesterov off) over the
parameter arena, for any pointer alignment and length, with host- or device-resident hyper-parameters, a bucket at a time under the
backward pass, on a launch tape, in a captured hipGraph, across a checkpoint, and from train.py's command line (--sgd)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
import supervised_dispnet_amd.loss_functions as LF  # noqa: E402
import supervised_dispnet_amd.models as models  # noqa: E402
from supervised_dispnet_amd import _lib, engine  # noqa: E402
from supervised_dispnet_amd.functional import reciprocal  # noqa: E402
from supervised_dispnet_amd.optim import FusedSGD  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [(64, 3, 3, 3), (64,), (17,), (128, 64, 3, 3), (1, 16, 3, 3)]       # (17,): a padded arena slice


def close(name, got, want, rtol=1e-6, atol_rel=1e-7):
    """The project's optimizer tolerance (tests/test_gpu_kernels.py::test_fused_adam_matches_torch_adam)."""
    got = got.detach().float().cpu()
    want = want.detach().float().cpu()
    assert got.shape == want.shape, "%s: shape %s vs %s" % (name, tuple(got.shape), tuple(want.shape))
    scale = float(want.abs().max()) + 1e-30
    err = (got - want).abs()
    tol = atol_rel * scale + rtol * want.abs()
    bad = err > tol
    if bad.any():
        idx = np.unravel_index(int(torch.argmax(err - tol)), got.shape)
        raise AssertionError("%s: %d/%d elements off; worst at %s got %.7g want %.7g (max|want| %.4g, max err %.4g)" % (
            name, int(bad.sum()), got.numel(), idx, float(got[idx]), float(want[idx]), scale, float(err.max())))


def _grad(p, it):
    return torch.randn(p.shape, generator=torch.Generator().manual_seed(it * 100 + p.numel())) * 10 ** (it - 1)


def _buffer_of(opt, q):
    """The slice of the flat momentum buffer that belongs to parameter q."""
    o = opt.arena.offsets[[id(p) for p in opt.arena.params].index(id(q))]
    return opt.momentum_buffer[o:o + q.numel()].view(q.shape)


@pytest.mark.parametrize("lr,momentum,wd", [(1e-2, 0.9, 0.0), (1e-2, 0.9, 5e-4), (1e-4, 0.9, 5e-4), (1e-2, 0.0, 5e-4)])
def test_fused_sgd_matches_torch_sgd(lr, momentum, wd):
    torch.manual_seed(0)
    ref_p = [torch.randn(s).requires_grad_() for s in SHAPES]
    dev_p = [nn.Parameter(p.detach().clone().to(DEV)) for p in ref_p]
    opt_ref = torch.optim.SGD(ref_p, lr=lr, momentum=momentum, weight_decay=wd)
    opt = FusedSGD(dev_p, lr=lr, momentum=momentum, weight_decay=wd)
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"], g["dampening"], g["nesterov"]) == (lr, momentum, wd, 0, False)
    assert opt.momentum_buffer.shape == opt.arena.flat_p.shape and not bool(opt.momentum_buffer.any())
    epoch = engine.PARAM_EPOCH
    for it in range(3):
        for p, q in zip(ref_p, dev_p):
            gr = _grad(p, it)
            p.grad = gr.clone()
            q._dn_grad_view.copy_(gr.to(DEV))
        opt_ref.step()
        opt.step()
        assert engine.PARAM_EPOCH == epoch + it + 1
        if momentum == 0:
            # the buffer-less form of torch: same parameters after EVERY step, while the buffer here holds the last gradient (+ wd * p)
            for p, q in zip(ref_p, dev_p):
                close("sgd p, step %d" % it, q.detach(), p.detach())
    for p, q in zip(ref_p, dev_p):
        close("sgd p", q.detach(), p.detach())
        if momentum != 0:
            close("sgd momentum_buffer", _buffer_of(opt, q), opt_ref.state[p]["momentum_buffer"])
    pad = torch.ones(opt.arena.numel, dtype=torch.bool, device=DEV)
    for q, o in zip(opt.arena.params, opt.arena.offsets):
        pad[o:o + q.numel()] = False
    assert int(pad.sum()) == 3 and not bool(opt.momentum_buffer[pad].any()) and not bool(opt.arena.flat_p[pad].any())


OFFSETS = [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3),          # one offset for p, g, buf: scalar head, 16-byte body, scalar tail
           (0, 1, 2), (3, 3, 1), (0, 0, 2)]                     # offsets that disagree: every element on the scalar lane
SENTINEL = 12345.0


def test_sgd_step_any_alignment_and_length_is_bitwise_the_aligned_update():
    gen = torch.Generator().manual_seed(7)
    lr, momentum, wd, scale = 1e-2, 0.9, 5e-4, 0.5
    for n in (1, 3, 4, 5, 255, 256, 257, 1023, 4099):
        vals = [torch.randn(n, generator=gen).to(DEV) for _ in range(3)]
        want = None
        for offs in OFFSETS:
            base = [torch.full((n + 16,), SENTINEL, device=DEV) for _ in range(3)]
            assert all(b.data_ptr() % 16 == 0 for b in base)
            view = [b[4 + k:4 + k + n] for b, k in zip(base, offs)]
            for v, x in zip(view, vals):
                v.copy_(x)
            for _ in range(2):                                     # the second step reads the buffer the first one wrote
                _lib.call("dn_sgd_step", view[0].data_ptr(), view[1].data_ptr(), view[2].data_ptr(), n, lr, momentum, wd, scale,
                          engine._stream())
            got = (view[0].clone(), view[2].clone())
            if want is None:
                want = got
                assert not torch.equal(want[0], vals[0]) and not torch.equal(want[1], vals[2])
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (n, offs)
            assert torch.equal(view[1], vals[1]), (n, offs)        # the gradient is read only
            for b, k in zip(base, offs):
                guard = torch.cat([b[:4 + k], b[4 + k + n:]])
                assert torch.equal(guard, torch.full_like(guard, SENTINEL)), (n, offs)


def test_sgd_step_refuses_null_pointers_and_empty_ranges():
    t = torch.zeros(8, device=DEV)
    h = torch.zeros(2, dtype=torch.float64, device=DEV)
    p, s = t.data_ptr(), engine._stream()
    for args in ((0, p, p, 8), (p, 0, p, 8), (p, p, 0, 8), (p, p, p, 0), (p, p, p, -4)):
        with pytest.raises(_lib.DispnetHipError, match="dn_sgd_step: bad argument"):
            _lib.call("dn_sgd_step", *args, 0.1, 0.9, 0.0, 1.0, s)
    for args in ((0, p, p, 8, h.data_ptr()), (p, 0, p, 8, h.data_ptr()), (p, p, 0, 8, h.data_ptr()), (p, p, p, 0, h.data_ptr()),
                 (p, p, p, 8, 0)):
        with pytest.raises(_lib.DispnetHipError, match="dn_sgd_step_dev: bad argument"):
            _lib.call("dn_sgd_step_dev", *args, 0.0, 1.0, s)
    torch.cuda.synchronize()
    assert not bool(t.any())


def test_host_and_device_hyper_parameters_agree_bitwise():
    torch.manual_seed(1)
    init = [torch.randn(s) for s in SHAPES]
    opts = []
    for on in (False, True):
        ps = [nn.Parameter(p.clone().to(DEV)) for p in init]
        opts.append((ps, FusedSGD(ps, lr=1e-2, momentum=0.9, weight_decay=5e-4).capturable(on)))
    (_, opt_h), (_, opt_d) = opts
    assert opt_h._dev is None and opt_d._dev["hyper"].dtype == torch.float64 and opt_d._dev["hyper"].tolist() == [1e-2, 0.9]
    for it in range(6):
        if it == 2:                                                # a scheduler, through set_lr
            for _, o in opts:
                o.set_lr(3e-3)
            assert opt_d._dev["hyper"].tolist() == [3e-3, 0.9]
        if it == 4:                                                # ... and one that writes the parameter group as torch's do
            for _, o in opts:
                o.param_groups[0]["lr"] = 7e-4
        for ps, o in opts:
            for q in ps:
                q._dn_grad_view.copy_(_grad(q, it % 3).to(DEV))
            o.step(grad_scale=0.5)
        assert torch.equal(opt_h.arena.flat_p, opt_d.arena.flat_p), it
        assert torch.equal(opt_h.momentum_buffer, opt_d.momentum_buffer), it
    assert opt_d._dev["hyper"].tolist() == [7e-4, 0.9]
    assert [t.data_ptr() for t in opt_d.tape_state()] == [opt_d.arena.flat_p.data_ptr(), opt_d.momentum_buffer.data_ptr()]


def _make(sd0=None):
    torch.manual_seed(0)
    net = models.Disp_vgg_BN(datasets="kitti", with_classifier=False)
    bench._quiet_init(net)
    if sd0 is not None:
        net.load_state_dict(sd0)
    net.to(DEV).train()
    opt = FusedSGD(net._hot_parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4, production_order=net._grad_production_order())
    return net, opt


def _bn_and_params_equal(net_a, net_b):
    sa, sb = net_a.state_dict(), net_b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("taped", [False, True], ids=["eager", "taped"])
def test_sgd_per_bucket_under_the_backward_pass_is_bitwise_the_single_update(taped):
    """FusedSGD.overlap_backward: apply_range over the buckets a GradReducer watches (one rank: nothing is exchanged), enqueued as
    the buckets complete, equals one whole-arena step -- parameters, momentum buffer and every loss, eagerly and on a launch tape."""
    from supervised_dispnet_amd.distributed import GradReducer
    from supervised_dispnet_amd.graph import TapedStep, backward
    batches = [bench.synthetic_batch(4, 64, 96, DEV, seed) for seed in range(4)]
    net_a, opt_a = _make()
    sd0 = copy.deepcopy({k: v.detach().cpu().clone() for k, v in net_a.state_dict().items()})
    net_b, opt_b = _make(sd0)
    opt_a.capturable(True)
    opt_b.capturable(True)
    red = GradReducer(opt_b.arena, bucket_bytes=8 << 20, comm="torch")
    assert red.path == "none" and len(red.buckets) >= 4
    opt_b.overlap_backward(red)
    img, gt = batches[0][0].clone(), batches[0][1].clone()

    def step_a(x, y):
        depth = [reciprocal(d) for d in net_a(x)]
        loss = LF.l1_loss(y, depth, "kitti")
        opt_a.zero_grad()
        backward(loss)
        opt_a.step()
        return loss

    def step_b():
        engine.GradSink.reducer = red
        try:
            depth = [reciprocal(d) for d in net_b(img)]
            loss = LF.l1_loss(gt, depth, "kitti")
            opt_b.zero_grad()
            backward(loss)
            opt_b.step(grad_scale=red.finish())
        finally:
            engine.GradSink.reducer = None
        return loss

    with pytest.raises(RuntimeError, match="FusedSGD.overlap_backward: step\\(\\) without a backward pass"):
        opt_b.step()
    f = TapedStep(step_b, optimizer=opt_b, warmup=1, static_inputs=(img, gt)) if taped else step_b
    if taped:
        f.capture()                    # one warm-up + the recorded step on batch 0
        for _ in range(2):
            step_a(*batches[0])
        assert f.segments == 1
    for x, y in batches:
        img.copy_(x)
        gt.copy_(y)
        lb = f().clone()
        la = step_a(x, y).clone()
        assert torch.isfinite(la).all() and torch.equal(la, lb)
    torch.cuda.synchronize()
    assert torch.equal(opt_a.arena.flat_p, opt_b.arena.flat_p)
    assert torch.equal(opt_a.momentum_buffer, opt_b.momentum_buffer) and bool(opt_a.momentum_buffer.any())


def test_launch_tape_replay_is_bitwise_the_eager_sgd_step():
    """graph.TapedStep with FusedSGD at 2x64x96: no bias correction, so nothing is evaluated in two places -- losses, parameters, momentum
    buffer and BatchNorm buffers after 8 steps on changing batches are EQUAL, with freed pool memory scribbled over between replays."""
    from supervised_dispnet_amd.graph import TapedStep, backward
    batches = [bench.synthetic_batch(2, 64, 96, DEV, seed) for seed in range(5)]
    net_e, opt_e = _make()
    sd0 = copy.deepcopy({k: v.detach().cpu().clone() for k, v in net_e.state_dict().items()})
    net_t, opt_t = _make(sd0)
    img, gt = batches[0][0].clone(), batches[0][1].clone()

    def step_t():
        depth = [reciprocal(d) for d in net_t(img)]
        loss = LF.l1_loss(gt, depth, "kitti")
        opt_t.zero_grad()
        backward(loss)
        opt_t.step()
        return loss

    def step_e(x, y):
        depth = [reciprocal(d) for d in net_e(x)]
        loss = LF.l1_loss(y, depth, "kitti")
        opt_e.zero_grad()
        loss.backward()
        opt_e.step()
        return loss

    ts = TapedStep(step_t, optimizer=opt_t, warmup=2, static_inputs=(img, gt))
    ts.capture()                       # 2 warm-up steps + the recorded one: three real steps on batch 0
    for _ in range(3):
        step_e(*batches[0])
    assert ts.launches > 100 and ts.fences > 10 and ts.segments == 1
    assert opt_t._dev is not None and opt_e._dev is None            # device-side hyper-parameters on the tape, host-side eagerly
    losses_t, losses_e = [], []
    for x, y in batches[1:]:
        img.copy_(x)
        gt.copy_(y)
        losses_t.append(ts().clone())
        losses_e.append(step_e(x, y).clone())
    # scribble over freed memory of the regular pool between replays: the tape's buffers live in their own pool
    junk = [torch.full((1 << 20,), float("nan"), device=DEV) for _ in range(8)]
    del junk
    img.copy_(batches[0][0])
    gt.copy_(batches[0][1])
    losses_t.append(ts().clone())
    losses_e.append(step_e(*batches[0]).clone())
    torch.cuda.synchronize()
    for lt, le in zip(losses_t, losses_e):
        assert torch.isfinite(lt).all() and torch.equal(lt, le), (lt, le)
    assert torch.equal(opt_t.arena.flat_p, opt_e.arena.flat_p)
    assert torch.equal(opt_t.momentum_buffer, opt_e.momentum_buffer)
    _bn_and_params_equal(net_t, net_e)
    ts.close()


def test_graph_replay_is_bitwise_the_eager_sgd_step():
    """graph.GraphedStep (hipGraph capture) of one FusedSGD step at 2x64x96, replayed over three changing batches."""
    from supervised_dispnet_amd.graph import GraphedStep
    batches = [bench.synthetic_batch(2, 64, 96, DEV, seed) for seed in range(3)]
    net_e, opt_e = _make()
    sd0 = copy.deepcopy({k: v.detach().cpu().clone() for k, v in net_e.state_dict().items()})
    net_g, opt_g = _make(sd0)
    img, gt = batches[0][0].clone(), batches[0][1].clone()          # the graph's static input buffers

    def step_g():
        depth = [reciprocal(d) for d in net_g(img)]
        loss = LF.l1_loss(gt, depth, "kitti")
        opt_g.zero_grad()
        loss.backward()
        opt_g.step()
        return loss

    def step_e(x, y):
        depth = [reciprocal(d) for d in net_e(x)]
        loss = LF.l1_loss(y, depth, "kitti")
        opt_e.zero_grad()
        loss.backward()
        opt_e.step()
        return loss

    gs = GraphedStep(step_g, optimizer=opt_g, warmup=2, static_inputs=(img, gt))
    gs.capture()                       # two warm-up steps on batch 0 are real; the captured one never runs
    for _ in range(2):
        step_e(*batches[0])
    for x, y in batches:
        img.copy_(x)
        gt.copy_(y)
        lg = gs().clone()
        le = step_e(x, y).clone()
        assert torch.isfinite(lg).all() and torch.equal(lg, le), (lg, le)
    torch.cuda.synchronize()
    assert torch.equal(opt_g.arena.flat_p, opt_e.arena.flat_p)
    assert torch.equal(opt_g.momentum_buffer, opt_e.momentum_buffer)
    _bn_and_params_equal(net_g, net_e)


def test_resume_from_own_and_from_torch_sgd_state():
    torch.manual_seed(2)
    lr, momentum, wd = 1e-2, 0.9, 5e-4
    ref_p = [torch.randn(s).requires_grad_() for s in SHAPES]
    dev_p = [nn.Parameter(p.detach().clone().to(DEV)) for p in ref_p]
    opt_ref = torch.optim.SGD(ref_p, lr=lr, momentum=momentum, weight_decay=wd)
    opt = FusedSGD(dev_p, lr=lr, momentum=momentum, weight_decay=wd)

    def step(o, ps, it):
        for q in ps:
            if q.is_cuda:
                q._dn_grad_view.copy_(_grad(q, it % 3).to(DEV))
            else:
                q.grad = _grad(q, it % 3)
        o.step()

    for it in range(2):
        step(opt, dev_p, it)
        step(opt_ref, ref_p, it)
    # (a) this class's own form into a fresh optimizer over copies of the parameters: two more steps, bit for bit
    sd = opt.state_dict()
    assert set(sd) == {"momentum_buffer", "param_groups"} and sd["momentum_buffer"].shape == (opt.arena.numel,)
    assert sd["momentum_buffer"].data_ptr() != opt.momentum_buffer.data_ptr()
    assert sd["param_groups"] == [{"lr": lr, "momentum": momentum, "weight_decay": wd, "dampening": 0, "nesterov": False}]
    new_p = [nn.Parameter(q.detach().clone()) for q in dev_p]
    opt2 = FusedSGD(new_p, lr=lr, momentum=momentum, weight_decay=wd)
    opt2.load_state_dict(sd)
    # (b) torch.optim.SGD's state after the same two steps on the CPU, into an arena that orders the parameters differently
    tp = [nn.Parameter(p.detach().clone().to(DEV)) for p in ref_p]
    opt3 = FusedSGD(tp, lr=lr, momentum=momentum, weight_decay=wd, production_order=[tp[i] for i in (3, 0, 4, 2, 1)])
    assert [id(p) for p in opt3.arena.params] != [id(p) for p in tp]
    opt3.load_state_dict(opt_ref.state_dict())
    for it in range(2, 4):
        step(opt, dev_p, it)
        step(opt2, new_p, it)
        assert torch.equal(opt.arena.flat_p, opt2.arena.flat_p) and torch.equal(opt.momentum_buffer, opt2.momentum_buffer)
    step(opt3, tp, 2)
    step(opt_ref, ref_p, 2)
    for p, q in zip(ref_p, tp):
        close("resumed p", q.detach(), p.detach())
        close("resumed momentum_buffer", _buffer_of(opt3, q), opt_ref.state[p]["momentum_buffer"])
    with pytest.raises(ValueError, match="arena has"):
        opt2.load_state_dict({"momentum_buffer": torch.zeros(5)})


def _run_train(tmp_path, extra, epochs=2, n=16, b=4):
    import train
    train.main(["SYN", "--synthetic", str(n), "-b", str(b), "--epochs", str(epochs), "--img-height", "64", "--img-width", "96",
                "--lr", "1e-3", "--save-root", str(tmp_path), "--print-freq", "100"] + extra)
    runs = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path) for f in fs]
    full = [r for r in runs if r.endswith("progress_log_full.csv")][0]
    rows = [l.split("\t") for l in open(full).read().strip().splitlines()]
    assert len(rows) == 1 + epochs * (n // b)
    vals = np.array([[float(v) for v in r] for r in rows[1:]])
    assert np.isfinite(vals).all()
    ckpt = [r for r in runs if r.endswith("dispnet_checkpoint.pth.tar")]
    assert len(ckpt) == 1
    return vals, torch.load(ckpt[0], map_location="cpu"), ckpt[0]


def test_train_cli_sgd_on_the_launch_tape_equals_the_eager_run(tmp_path, capsys):
    """train.py --sgd: FusedSGD on the arena, on the launch tape by default; the same losses and weights as --no-tape, exactly (there is
    no bias correction to evaluate in two places); the checkpoint carries the flat momentum buffer and a second run restores it."""
    args = ["--network", "disp_vgg_BN", "--with-gt", "--loss", "L1", "--sgd", "--seed", "3"]
    ve, sde, _ = _run_train(tmp_path / "eager", args + ["--no-tape"])
    out = capsys.readouterr().out
    assert "=> setting sgd solver" in out and "--tape:" not in out
    vt, sdt, ckpt = _run_train(tmp_path / "tape", args)                                  # (no flag: the tape is the default)
    out = capsys.readouterr().out
    assert "=> setting sgd solver" in out and "=> setting adam solver" not in out
    assert "--tape:" in out and "bit for bit" in out, out[-600:]
    assert "eager launches (" not in out
    assert vt.shape == ve.shape and np.array_equal(vt, ve), (vt[:, 0], ve[:, 0])
    for k, v in sde["state_dict"].items():
        assert torch.equal(v, sdt["state_dict"][k]), k
    arena_numel = sum((p.numel() + 3) // 4 * 4 for p in models.Disp_vgg_BN(datasets="kitti", with_classifier=False)._hot_parameters())
    mb = sdt["optimizer"]["momentum_buffer"]
    assert mb.dim() == 1 and mb.numel() == arena_numel and bool(mb.any())
    assert torch.equal(mb, sde["optimizer"]["momentum_buffer"])
    _run_train(tmp_path / "resumed", args + ["--pretrained-disp", ckpt], epochs=1, n=4)
    out = capsys.readouterr().out
    assert "=> setting sgd solver" in out and "not restored" not in out


def _make_sgd_net(dev):
    """tests/test_gpu_two_ranks.py::_make_net with FusedSGD in FusedAdam's place."""
    torch.manual_seed(0)
    net = models.Disp_vgg_BN(datasets="kitti", with_classifier=False)
    bench._quiet_init(net)
    net.to(dev).train()
    opt = FusedSGD(net._hot_parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4, production_order=net._grad_production_order())
    return net, opt


def _two_rank_worker(rank, world, port, out_dir):
    import test_gpu_two_ranks as T
    T._make_net = _make_sgd_net
    T._worker(rank, world, port, "L1", out_dir, True)


def test_two_ranks_with_sgd_per_bucket_equal_the_single_process_step(tmp_path, monkeypatch):
    """The two-rank launcher of tests/test_gpu_two_ranks.py with FusedSGD: two processes on one GPU, gloo, the step on a launch tape cut
    at every gradient bucket, each bucket's SGD update right behind its all-reduce (overlap_backward), three steps -- against ONE process
    stepping the concatenated batch (two replicas, gradients added, one update): l1_loss, so bit for bit as in that file."""
    import torch.multiprocessing as mp
    import test_gpu_two_ranks as T
    ctx = mp.get_context("spawn")
    port = T._free_port()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    r0 = torch.load(os.path.join(str(tmp_path), "rank0.pt"))
    r1 = torch.load(os.path.join(str(tmp_path), "rank1.pt"))
    assert torch.equal(r0["g1"], r1["g1"]) and torch.equal(r0["p"], r1["p"])
    assert r0["log"] == r1["log"] and r0["scale"] == 0.5
    assert len([e for e in r0["log"] if e[0] == "bucket"]) // T.STEPS >= 4
    monkeypatch.setattr(T, "_make_net", _make_sgd_net)
    p_ref, _g_ref, l_ref = T._single_process_reference("L1")
    assert r1["losses"] == l_ref
    assert torch.equal(r0["p"], p_ref), float((r0["p"] - p_ref).abs().max())
